"""The restatement K24 (az_result_images, az_result_img.hip) is compared with, byte for byte: the six result images of a test
batch in numpy float32, following matplotlib's Normalize.__call__ and Colormap.__call__(bytes=True) step by step, the cases
the CPU and GPU tests share, and the mutants that show the cases can tell a wrong rule from the right one.  Test
infrastructure: numpy only, never the product path.  The restatement itself is held against matplotlib's own plt.imsave:
tests/golden/g16_result_images.npz (tools/make_result_image_goldens.py) and, where matplotlib is installed, the live call.

The viridis table is data: it is read from the goldens file (and compared there with csrc/az_viridis_table.h)."""
import os
import re

import numpy as np

from tests import _gt_prep_ref as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "g16_result_images.npz")
HEADER = os.path.join(REPO, "activezero_amd", "csrc", "az_viridis_table.h")
PANELS = ("pred_disp", "gt_disp", "pred_disp_abs_err_cmap", "pred_depth", "gt_depth", "pred_depth_abs_err_cmap")  # save_img's order
VIRIDIS_PANELS = (0, 1, 3, 4)
INPUTS = ("pred", "view", "gt_disp", "gt_depth", "mask", "focal", "baseline", "max_disp")
RED = np.array([255, 0, 0, 255], np.uint8)
F = np.float32
# each must change a byte of the committed cases -- but for "no_256", which cannot: see test_result_images_cpu.py
MUTANTS = ("recip", "round", "no_256", "swap", "bad_from_mask", "nan_red", "nan_first", "one_flag", "depth_assoc", "fma",
           "fma_est", "legend_before_mask", "alpha_from_mask")


def header_table():
    """uint8 [256,3] as csrc/az_viridis_table.h states it"""
    with open(HEADER) as f:
        body = f.read().split("= {", 1)[1]
    rows = re.findall(r"\{(\d+), (\d+), (\d+)\}", body)
    return np.array(rows, dtype=np.int64).astype(np.uint8)


_table = None


def table():
    """uint8 [256,4]: matplotlib's viridis as bytes, alpha 255 (from the goldens file)"""
    global _table
    if _table is None:
        rgb = np.load(GOLDEN)["viridis_table"]
        _table = np.concatenate([rgb, np.full((256, 1), 255, np.uint8)], 1)
    return _table


def _bad(x, on, mutant):
    v = np.where(on, x, F(-1))
    return v, (~on if mutant == "bad_from_mask" else v == F(-1))


def _viridis(v, bad, vmax, any_bad, tab, mutant):
    """one image [H,W] -> uint8 [H,W,4]; v, bad from _bad; any_bad: np.ma.is_masked of this image"""
    vmax = F(vmax)
    with np.errstate(all="ignore"):
        xa = (v * (F(1) / vmax) if mutant == "recip" else v / vmax) * F(256)
        if mutant != "no_256":
            xa[xa == F(256)] = F(255)
        nan, under, over = np.isnan(xa), xa < 0, xa >= F(256)
        inner = np.where(nan | under | over, F(0), xa)
        idx = (np.minimum(np.rint(inner), 255) if mutant == "round" else inner).astype(np.int64)
    if mutant == "swap":
        under, over = over, under
    idx[under], idx[over] = 0, 255
    img = tab[idx]
    nan_red = {"nan_red": True, "nan_first": False}.get(mutant, not any_bad)
    img[nan] = RED if nan_red else tab[0]
    img[bad] = RED
    return img


def _error(kind, e_scaled, on, mutant):
    """one image: the scaled error [H,W] -> uint8 [H,W,4]"""
    rgb = np.array(G.RGB, np.uint8)
    cls = G.classes(e_scaled, kind)
    cls[~on] = -1
    img = np.zeros(cls.shape + (4,), np.uint8)
    img[..., 3] = 255
    img[cls >= 0, :3] = rgb[cls[cls >= 0]]
    for i in range(11):  # the legend; numpy slices clip it to the image
        img[:10, 20 * i:20 * i + 20, :3] = rgb[i]
    if mutant == "legend_before_mask":
        img[~on, :3] = 0
    return img


def result_images(pred, gt_disp, gt_depth, mask, focal, baseline, max_disp, depth_hi=1.25, disp_abs_thres=3.0,
                  disp_rel_thres=0.05, depth_scale=1000.0, depth_abs_thres=1.0, mutant=None):
    """pred, gt_disp, gt_depth [B,1,H,W] float32, mask [B,1,H,W] bool / uint8, focal, baseline [B] float32 ->
    (uint8 [B,6,H,W,4], flags int32 [B]).  focal x baseline is one float32 product, as test.py:209 makes it."""
    assert mutant is None or mutant in MUTANTS
    tab = table()
    B, _, H, W = pred.shape
    out, flags = np.zeros((B, 6, H, W, 4), np.uint8), np.zeros(B, np.int32)
    for b in range(B):
        pd, gd, gz, on = pred[b, 0].astype(F), gt_disp[b, 0].astype(F), gt_depth[b, 0].astype(F), mask[b, 0] != 0
        fb = F(F(focal[b]) * F(baseline[b]))
        with np.errstate(all="ignore"):
            pz = F(focal[b]) * (F(baseline[b]) / pd) if mutant == "depth_assoc" else fb / pd
            maps = {0: (pd, max_disp), 1: (gd, max_disp), 3: (pz, depth_hi), 4: (gz, depth_hi)}
            vb = {m: _bad(x, on, mutant) for m, (x, _) in maps.items()}
            for m in VIRIDIS_PANELS:
                flags[b] |= int(vb[m][1].any()) << m
            for m, (_, vmax) in maps.items():
                any_bad = flags[b] != 0 if mutant == "one_flag" else bool(flags[b] >> m & 1)
                out[b, m] = _viridis(vb[m][0], vb[m][1], vmax, any_bad, tab, mutant)
            out[b, 2] = _error("disp", G.scaled_error(pd, gd, "disp", disp_abs_thres, disp_rel_thres), on, mutant)
            s = F(depth_scale)
            if mutant == "fma":  # gt * s - fl(est * s) in one rounding, emulated in float64 (a 24 x 24 bit product is exact)
                e = np.abs(gz.astype(np.float64) * np.float64(s) - np.float64(pz * s)).astype(F)
            elif mutant == "fma_est":
                e = np.abs(np.float64(gz * s) - pz.astype(np.float64) * np.float64(s)).astype(F)
            else:
                e = np.abs(gz * s - pz * s)
            out[b, 5] = _error("depth", e / F(depth_abs_thres), on, mutant)
        if mutant == "alpha_from_mask":
            out[b, :, :, :, 3] = np.where(on, 255, 0)
    return out, flags


# ---- the cases ---------------------------------------------------------------------------------------------------------
FOCAL, BASELINE = F(446.31), F(0.055)


def pred_view(case):
    """the [B,1,H,W] view of the stored prediction: rows from view[0], the first W columns (test.py:208's crop)"""
    y0, h, w = (int(v) for v in case["view"])
    return case["pred"][:, :, y0:y0 + h, :w]


def run_case(case, **kw):
    return result_images(pred_view(case), case["gt_disp"], case["gt_depth"], case["mask"], case["focal"], case["baseline"],
                         float(case["max_disp"]), **kw)


def _case(pred, gt_disp, gt_depth, mask, focal=None, baseline=None, max_disp=192.0, pad=(0, 0)):
    B, _, H, W = gt_disp.shape
    stored = np.full((B, 1, H + pad[0], W + pad[1]), F(7777.0))  # what a kernel that ignores the strides would read
    stored[:, :, pad[0]:, :W] = pred
    return {"pred": stored.astype(F), "view": np.array([pad[0], H, W], np.int32), "gt_disp": gt_disp.astype(F),
            "gt_depth": gt_depth.astype(F), "mask": np.ascontiguousarray(mask).astype(np.uint8),
            "focal": np.full(B, FOCAL) if focal is None else np.asarray(focal, F),
            "baseline": np.full(B, BASELINE) if baseline is None else np.asarray(baseline, F), "max_disp": F(max_disp)}


def random_maps(seed, B, H, W, masked=0.3, focal=None, baseline=None, quantum=True):
    """(pred, gt_disp, gt_depth, mask, focal, baseline): gt_disp in (8, 190), pred = gt_disp +- 2^uniform(-6, 6.5) (some
    negative, some beyond 192), gt_depth = predicted depth +- 2^uniform(-13, -1) m, so every row of both error tables and
    under, inside and over of both colour ranges occur.  quantum: values on a grid (1/4 and 1/16 px, 2^-12 m), which keeps the
    committed arrays compressible; a quotient by 192 or 1.25 is inexact either way."""
    rng = np.random.default_rng(seed)
    focal = np.full(B, FOCAL) if focal is None else np.asarray(focal, F)
    baseline = np.full(B, BASELINE) if baseline is None else np.asarray(baseline, F)
    shape = (B, 1, H, W)
    gd = rng.uniform(8, 190, shape)
    pd = gd + rng.choice([-1.0, 1.0], shape) * 2.0 ** rng.uniform(-6, 6.5, shape)
    if quantum:
        gd, pd = np.round(gd * 4) / 4, np.round(pd * 16) / 16
    gd, pd = gd.astype(F), pd.astype(F)
    with np.errstate(all="ignore"):
        pz = (focal * baseline).astype(F).reshape(B, 1, 1, 1) / pd
    gz = np.where(np.isfinite(pz), pz, F(0.5)).astype(np.float64) + rng.choice([-1.0, 1.0], shape) * 2.0 ** rng.uniform(-13, -1, shape)
    if quantum:
        gz = np.round(gz * 4096) / 4096
    mask = rng.random(shape) >= masked
    return pd, gd, gz.astype(F), mask, focal, baseline


def _neighbours(t):
    t = np.asarray(t, F)
    return np.stack([np.nextafter(t, F(-np.inf)), t, np.nextafter(t, F(np.inf))], 1).reshape(-1)


def boundary_case():
    """2 x 777, mask on everywhere.  Row 0: pred_disp = gt_disp = j * 0.75, j = 0..256 -- the values whose quotient by 192 times
    256 is the integer j -- each with its float32 neighbour below and above, then +0, -0, +inf, -inf, a denormal, 3e38; gt_depth
    the same around j * 5 / 1024 (by 1.25 times 256: j).  Row 1: pred_disp = fb / (j * 5 / 1024), j = 1..256, with its
    neighbours, so the predicted depth lands on and beside the same bounds; then 0, -0, +-inf, +-denormal, 3e38, fb, NaN."""
    special = np.array([0.0, -0.0, np.inf, -np.inf, 1e-40, 3e38], F)
    j = np.arange(257)
    row_d = np.concatenate([_neighbours(F(0.75) * j.astype(F)), special])
    row_z = np.concatenate([_neighbours(j.astype(F) * F(5) / F(1024)), special])
    fb = F(FOCAL * BASELINE)
    with np.errstate(all="ignore"):
        d1 = np.concatenate([_neighbours(fb / (j[1:].astype(F) * F(5) / F(1024))),
                             np.array([0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, 3e38, fb, np.nan], F)])
        W = row_d.size
        assert W == 777 == d1.size
        rng = np.random.default_rng(2401)
        pz1 = fb / d1
    pred = np.stack([row_d, d1]).reshape(1, 1, 2, W)
    gt_disp = np.stack([row_d, (np.round(rng.uniform(8, 190, W) * 4) / 4).astype(F)]).reshape(1, 1, 2, W)
    gt_depth = np.stack([row_z, np.where(np.isfinite(pz1), pz1, F(0.5)).astype(F)]).reshape(1, 1, 2, W)
    return _case(pred, gt_disp, gt_depth, np.ones((1, 1, 2, W), bool))


def contraction_pairs(n=80, seed=2402):
    """(pred_disp, gt_depth) float32 [n] x2, found by search: pairs whose depth error 1000 gt - 1000 est falls in one table row
    when both products and the difference are rounded (the reference) and in ANOTHER when the difference is contracted with
    either product into an fma.  Half have gt = est exactly (the reference gives 0, row 0; an fma gives the product's
    rounding error, row 1 when it is >= 1e-5), half sit within a few ulp of an inner bound."""
    rng = np.random.default_rng(seed)
    fb, s = F(FOCAL * BASELINE), F(1000)
    bd = G.bounds("depth")
    d = rng.uniform(20, 120, 400000).astype(F)
    pz = fb / d
    k = rng.integers(2, 9, d.size)
    near = (pz.astype(np.float64) + bd[k].astype(np.float64) / 1000).astype(F)
    near = near.view(np.int32) + rng.integers(-3, 4, d.size).astype(np.int32)
    gz = np.where(np.arange(d.size) % 2 == 0, pz, near.view(F))

    def rows(e):
        return G.classes(e.astype(F), "depth")

    plain = rows(np.abs(gz * s - pz * s))
    fma_gt = rows(np.abs(gz.astype(np.float64) * 1000.0 - np.float64(pz * s)))
    fma_est = rows(np.abs(np.float64(gz * s) - pz.astype(np.float64) * 1000.0))
    hit = (plain != fma_gt) & (plain != fma_est) & (plain >= 0) & (fma_gt >= 0) & (fma_est >= 0)
    even, odd = np.flatnonzero(hit & (gz == pz))[:n // 2], np.flatnonzero(hit & (gz != pz))[:n - n // 2]
    assert even.size == n // 2 and odd.size == n - n // 2, (even.size, odd.size)
    pick = np.concatenate([even, odd])
    return d[pick], gz[pick]


def build_cases():
    """name -> case, in a fixed order; deterministic"""
    cases = {}
    one = np.full((1, 1, 1, 1), F(96.0))
    for name, on in (("one_on", True), ("one_off", False)):
        cases[name] = _case(one, one + F(2), np.full((1, 1, 1, 1), F(0.25)), np.full((1, 1, 1, 1), on))

    # B = 3, 12 x 231: the whole legend and 11 columns more, two rows below it, W % 4 = 3, one focal x baseline per image
    pd, gd, gz, mask, focal, baseline = random_maps(2403, 3, 12, 231, focal=[446.31, 446.31, 920.0], baseline=[0.055, 0.0545, 0.05])
    mask[0] = True  # image 0: fully valid, one NaN (red: nothing is masked) and one zero prediction (infinite depth)
    pd[0, 0, 11, 5], pd[0, 0, 10, 225] = np.nan, 0.0
    mask[1, 0, 11, 7], pd[1, 0, 11, 7] = True, np.nan  # image 1: masked pixels and a NaN (table[0])
    mask[1, 0, 3, 30:50] = False  # ... some of them under the legend
    mask[2] = True  # image 2: nothing masked, but one gt_disp IS -1: bad in panel 1 alone; its NaN stays red in panels 0 and 3
    gd[2, 0, 10, 3], pd[2, 0, 11, 100] = -1.0, np.nan
    cases["batch3"] = _case(pd, gd, gz, mask, focal, baseline)

    cases["clip"] = _case(*random_maps(2404, 1, 7, 53))  # the legend clipped both ways
    cases["boundary"] = boundary_case()
    # max_disp = 100: the quotient is inexact
    pd, gd, gz, mask, focal, baseline = random_maps(2405, 1, 5, 37, quantum=False)
    cases["md100"] = _case(pd * F(0.6), gd * F(0.6), gz, mask, focal, baseline, max_disp=100.0)

    # the contraction pairs, below the legend of a 12 x 40 image
    pd, gd, gz, mask, focal, baseline = random_maps(2406, 1, 12, 40)
    cd, cz = contraction_pairs(80)
    pd[0, 0, 10:], gz[0, 0, 10:], mask[0, 0, 10:] = cd.reshape(2, 40), cz.reshape(2, 40), True
    cases["contract"] = _case(pd, gd, gz, mask, focal, baseline)

    # a pitched prediction: stored [B,1,H+4,W+5], viewed from row 4
    cases["pitched"] = _case(*random_maps(2407, 2, 9, 30), pad=(4, 5))
    return cases


def golden_cases():
    """name -> (case, images uint8 [B,6,H,W,4] as plt.imsave wrote them) from the committed file"""
    z = np.load(GOLDEN)
    names = []
    for k in z.files:
        if "/" in k and k.split("/")[0] not in names:
            names.append(k.split("/")[0])
    return {n: ({k: z[f"{n}/{k}"] for k in INPUTS}, z[f"{n}/images"]) for n in names}
