"""What tests/test_gpu_obj_metrics.py and tests/test_gpu_eval_mask.py hold K22 az_obj_metrics (csrc/az_obj_metrics.hip) and
K23 az_eval_mask (csrc/az_gt_prep.hip) to (numpy only), in the manner of tests/_reduce_ref.py.

K22 is restated through _reduce_ref.k12_metrics, the per-pixel restatement of K12's terms, applied to the pixels
mask != 0 && label == l of image b -- there is no second copy of the arithmetic here.  Rules, none fitted to GPU output:
  * counts (acc[b][l][1, 2, 4, 5, 6, 7]), present[b][l] and stats[0] are exact integers;
  * acc[b][l][0] is within sum_bound of fsum of its float32 terms, acc[b][l][3] within the contracted-multiply-add
    allowance of check_k12_metrics plus sum_bound (both from _reduce_ref); a cell with no masked pixel must be exactly 0;
  * NaN / inf are compared by class per (image, label): a NaN prediction spoils the two sums of its own cell only;
  * the wrappers' numbers (compute_obj_err, compute_obj_err_per_image, compute_err_metric_per_image) are within
    _reduce_ref.scalar_bound of the fp64 formula on the exact accumulators.
tests/test_obj_metrics_cpu.py proves on the CPU that these rules reject every wrong kernel of its list on these inputs.

Launch constants the sizes are built around (test_obj_metrics_cpu.py reads the source and fails when one moves):
  BLOCK = 256       `#define OM_BLOCK 256`
  GRID_CAP = 1024   `#define OM_GRID_CAP 1024`: workgroups over all images; an image gets min(ceil(P / 256),
                    max(1, 1024 / B)) of them, each striding over that image alone
  MAX_LABELS = 64   `#define AZ_OBJ_MAX_LABELS 64` (include/azhip.h)

Measured on an MI355X: the docstring of tests/test_gpu_obj_metrics.py, which prints the figures.
"""
import math

import numpy as np

from tests import _reduce_ref as R

F32 = np.float32
BLOCK, GRID_CAP, MAX_LABELS = 256, 1024, 64
N_CAP = GRID_CAP * BLOCK + BLOCK + 37  # B = 1: a second pass that only some workgroups take
SHAPES = tuple((1, 1, 1, n) for n in R.FLAT) + R.SHAPED + ((1, 1, 1, N_CAP),)
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
LAYOUTS = ("none", "constant", "every pixel", "runs of 3", "runs of 100", "blobs")
LAYOUT_L = {"none": 1, "constant": 3, "every pixel": 64, "runs of 3": 5, "runs of 100": 17, "blobs": 17}
OUTSIDE = (-1, None, -2 ** 31, 2 ** 31 - 1)  # None: L itself, the first label past the range


def blocks_per_image(B, P):
    return min((P + BLOCK - 1) // BLOCK, max(1, GRID_CAP // B))


# ---- inputs ------------------------------------------------------------------------------------------------------------
def labels(layout, shape, L):
    """int32 [n] (None for layout 'none'): the label of every pixel, laid out per image"""
    B, n, P = R._shape(shape)
    if layout == "none":
        return None
    i = np.arange(n) % P
    if layout == "constant":
        lab = np.full(n, 1)
    elif layout == "every pixel":  # 64 distinct labels in every wave
        lab = i % L
    elif layout == "runs of 3":    # runs straddle waves (64 is no multiple of 3)
        lab = (i // 3) % L
    elif layout == "runs of 100":  # ... and blocks
        lab = (i // 100 + np.arange(n) // P) % L
    else:                          # blobs of 5 x 7 pixels on the image's own rows
        W = shape[-1]
        lab = ((i // W // 5) * 3 + (i % W) // 7) % L
    return lab.astype(np.int32)


def obj_case(shape, seed, layout):
    """_reduce_ref.metrics_case (its special pixels sit on every threshold and on both sides of every image boundary) plus a
    label map and hostile pixels: labels outside [0, L) -- -1, L, INT_MIN, INT_MAX in turn, on masked pixels -- three pixels
    to either side of every position of _reduce_ref.special_positions (the positions themselves keep the threshold and
    focal-length pixels, which must stay counted); where the layout has several labels and the image 128 pixels, a NaN
    prediction on a masked pixel (it spoils the two sums of its own cell only) and a NaN prediction and ground truth on an
    unmasked pixel beside it (it spoils nothing)"""
    c = dict(R.metrics_case(shape, seed))
    L = LAYOUT_L[layout]
    lab = labels(layout, shape, L)
    n, P = c["n"], c["per_batch"]
    flat = {k: c[k].ravel().copy() for k in ("dg", "zg", "dp", "zp", "mask")}
    outside = []
    if lab is not None:
        k = 0
        for p in R.special_positions(n, P):
            for q in (p - 3, p + 3):
                if 0 <= q < n and q // P == p // P:
                    v = OUTSIDE[k % 4]
                    lab[q] = L if v is None else v
                    flat["mask"][q] = 1
                    outside.append(q)
                    k += 1
        if L > 1 and layout != "constant" and P >= 128:
            for b in range(c["B"]):
                q = b * P + P // 2 + 9
                flat["dp"][q], flat["zp"][q], flat["mask"][q] = F32(np.nan), F32(np.nan), 1
                flat["dp"][q + 1] = flat["dg"][q + 1] = flat["zp"][q + 1] = F32(np.nan)
                flat["mask"][q + 1] = 0
                lab[q] = lab[q + 1] = (b + 2) % L
    for k, v in flat.items():
        c[k] = v.reshape(shape)
    c.update(label=None if lab is None else lab.reshape(shape), L=L, layout=layout, outside=len(outside),
             name=f"{c['name']} {layout}")
    return c


def cases(shape_index):
    """(case, path name, explicit depth_pred or None) for one shape: every layout, both depth sources"""
    for k, layout in enumerate(LAYOUTS):
        c = obj_case(SHAPES[shape_index], 8100 + 10 * shape_index + k, layout)
        yield c, "fb", None
        yield c, "depth_pred", c["zp"]


# ---- K22 restated ------------------------------------------------------------------------------------------------------
def _merge(parts):
    if len(parts) == 1:
        return parts[0]
    return dict(dd=np.concatenate([r["dd"] for r in parts]), mm64=np.concatenate([r["mm64"] for r in parts]),
                mm_tol=np.concatenate([r["mm_tol"] for r in parts]),
                counts=[sum(r["counts"][k] for r in parts) for k in range(6)])


def k22(c, zp, defect=None):
    """(cells {(b, l): k12_metrics dict over mask != 0 && label == l of image b}, present [B][L], stats) -- or what one of
    the wrong kernels of tests/test_obj_metrics_cpu.py makes of the same inputs (`defect`)"""
    B, n, P, L = c["B"], c["n"], c["per_batch"], c["L"]
    dg, zg, dp, mask = (c[k].ravel() for k in ("dg", "zg", "dp", "mask"))
    zpf = None if zp is None else zp.ravel()
    lab = np.zeros(n, dtype=np.int64) if c["label"] is None else c["label"].ravel().astype(np.int64)
    i = np.arange(n)
    img, pix = i // P, i % P
    inside = (lab >= 0) & (lab < L)
    stats = int((~inside).sum())
    seen = np.ones(n, dtype=bool)
    on = mask != 0
    row, fb_img = img, img  # the image whose accumulator row / whose focal length a pixel goes to
    if defect == "mask_ignored":
        on = np.ones(n, dtype=bool)
    elif defect == "label_plus1":
        lab = lab - 1
        inside = (lab >= 0) & (lab < L)
    elif defect == "clamped":
        lab = np.where(inside, lab, L - 1)
        inside = np.ones(n, dtype=bool)
    elif defect == "wave_merge":  # a wave's 64 pixels all go to the label of its first pixel
        first = lab[i - pix % 64]
        lab = np.where(inside & (first >= 0) & (first < L), first, lab)
    elif defect == "fb0":
        fb_img = np.zeros(n, dtype=np.int64)
    elif defect == "image_boundary":  # flat 256-pixel blocks: a block belongs to the image of its first pixel
        row = (i // BLOCK * BLOCK) // P
    elif defect == "tail":
        seen = pix < P - P % BLOCK
    elif defect == "one_pass":
        seen = pix < blocks_per_image(B, P) * BLOCK
    k12_defect = defect if defect in ("ge0", "ge1", "ge2", "ge3", "ge4") else None
    present = np.zeros((B, L), dtype=np.int64)
    cells = {}
    counted = (on if defect == "present_masked" else np.ones(n, dtype=bool)) & inside & seen
    np.add.at(present, (row[counted], lab[counted]), 1)
    take = on & inside & seen
    key = (row * L + np.where(inside, lab, 0)) * B + fb_img
    order = np.flatnonzero(take)
    order = order[np.argsort(key[order], kind="stable")]
    bounds = np.flatnonzero(np.diff(key[order])) + 1
    groups = {}
    for g in np.split(order, bounds) if order.size else []:
        kk = int(key[g[0]])
        groups.setdefault(kk // B, []).append((kk % B, g))
    empty = np.zeros(0, dtype=F32)
    for b in range(B):
        for l in range(L):
            if defect == "last_dropped" and l == L - 1:
                present[b, l] = 0
                parts = []
            else:
                parts = groups.get(b * L + l, [])
            rs = [R.k12_metrics(dg[g], zg[g], dp[g], None if zpf is None else zpf[g], c["fb"][fb:fb + 1],
                                np.ones(g.size, dtype=np.uint8), 1 << 40, defect=k12_defect) for fb, g in parts]
            cells[b, l] = _merge(rs) if rs else dict(dd=empty, mm64=empty.astype(np.float64), mm_tol=empty.astype(np.float64),
                                                     counts=[0] * 6)
    return cells, present, stats


def k22_exact(c, zp, defect=None):
    """(acc [B][L][8], present, stats) of a kernel that sums exactly"""
    cells, present, stats = k22(c, zp, defect)
    acc = np.zeros((c["B"], c["L"], 8))
    for (b, l), r in cells.items():
        n = r["counts"]
        acc[b, l] = [R.fsum(r["dd"]), n[0], n[1], R.fsum(r["mm64"]), n[2], n[3], n[4], n[5]]
    return acc, present, np.array([stats])


def check_k22(got, c, zp, calls=1, what="az_obj_metrics"):
    """got = (acc, present, stats) after `calls` launches into zeroed outputs; returns the largest err / bound of the two sums"""
    acc, present, stats = got
    cells, want_present, want_stats = k22(c, zp)
    assert acc.shape == (c["B"], c["L"], 8) and present.shape == want_present.shape, what
    R._same_int(np.asarray(stats).ravel()[0], calls * want_stats, f"{what} stats[0]")
    worst = {"acc[0]": 0.0, "acc[3]": 0.0}
    for (b, l), r in cells.items():
        w = f"{what} {c['name']} image {b} label {l}"
        R._same_int(present[b, l], calls * want_present[b, l], f"{w} present")
        for slot, n in zip((1, 2, 4, 5, 6, 7), r["counts"]):
            R._same_int(acc[b, l, slot], calls * n, f"{w} acc[{slot}]")
        e0 = R.check_sum(float(acc[b, l, 0]), r["dd"], f"{w} acc[0]", calls)
        e3 = R.check_sum(float(acc[b, l, 3]), r["mm64"], f"{w} acc[3]", calls, extra=R.fsum(r["mm_tol"]))
        worst["acc[0]"], worst["acc[3]"] = max(worst["acc[0]"], e0), max(worst["acc[3]"], e3)
    return worst


# ---- the wrappers' formulas --------------------------------------------------------------------------------------------
def _mean(terms, n, own=0.0):
    """(fsum(terms) / n, bound) -- (NaN, 0) over nothing"""
    if n == 0:
        return math.nan, 0.0
    v = R.fsum(terms) / n
    return v, R.scalar_bound(v, (R.sum_bound(terms) + own) / n) if math.isfinite(v) else 0.0


def obj_err_scalars(c, zp, per_image):
    """the four arrays of compute_obj_err (per_image False: the batch is one set of pixels) or compute_obj_err_per_image
    (the sum over the images of each image's mean; count = images the object appears in): ([L] values, [L] bounds) x 3
    and the counts"""
    cells, present, stats = k22(c, zp)
    assert stats == 0
    B, L = c["B"], c["L"]
    vals, lims, count = np.zeros((3, L)), np.zeros((3, L)), np.zeros(L)
    units = [[b] for b in range(B)] if per_image else [list(range(B))]
    for unit in units:
        for l in range(L):
            if not sum(present[b, l] for b in unit):
                continue
            r = _merge([cells[b, l] for b in unit])
            n = r["counts"][5]
            for k, (v, lim) in enumerate((_mean(r["dd"], n), _mean(r["mm64"], n, R.fsum(r["mm_tol"])),
                                          (r["counts"][3] / n if n else math.nan, 0.0))):
                vals[k, l] += v
                lims[k, l] += lim + 4 * R.U * abs(v if math.isfinite(v) else 0.0)
            count[l] += 1
    return vals, lims, count


def image_slice(c, zp, b):
    """the arguments of _reduce_ref.metrics_scalars / check_k12_metrics for image b alone"""
    f = lambda a: None if a is None else a[b:b + 1]
    return f(c["dg"]), f(c["zg"]), f(c["dp"]), f(zp), c["fb"][b:b + 1], f(c["mask"]), c["per_batch"]


# ---- K23 restated ------------------------------------------------------------------------------------------------------
def nearest_src(n_out, n_in):
    """ATen's legacy "nearest" source index for an output size: min((int)floorf(dst * scale), in - 1), scale = (float)in / out"""
    scale = F32(n_in) / F32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=F32) * scale).astype(np.int64), n_in - 1)


def eval_mask(disp_l, depth_l, max_disp, exclude_bg=True, robot=None, realsense=None, depth_hi=1.25):
    """(mask bool [B,1,H,W], count): disp_l, depth_l float32 [B,1,H,W]; robot / realsense [B,h,w] float32 or float64, read in
    their own type at the nearest source indices; (int) truncates toward zero"""
    B, _, H, W = disp_l.shape
    with np.errstate(invalid="ignore"):
        on = (disp_l > F32(0)) & (disp_l < F32(max_disp))
        if exclude_bg:
            on &= (depth_l > F32(0)) & (depth_l < F32(depth_hi))
        if robot is not None:
            r = robot[:, nearest_src(H, robot.shape[1])][:, :, nearest_src(W, robot.shape[2])]
            on &= (np.trunc(r) == 0)[:, None]
        if realsense is not None:
            s = realsense[:, nearest_src(H, realsense.shape[1])][:, :, nearest_src(W, realsense.shape[2])]
            on &= (s > 0)[:, None]
    return on, int(on.sum())


def eval_mask_case(B, H, W, aux_hw, dtype, seed):
    """disp_l, depth_l, robot, realsense: a third of the pixels fails each term; the exclusive bounds, -0, NaN and the robot
    values around the truncation (0.999..., 1, -0.5, -0.999..., -1) are all present"""
    rng = np.random.default_rng(seed)
    disp = rng.uniform(-20.0, 260.0, (B, 1, H, W)).astype(F32)
    depth = rng.uniform(-0.2, 1.8, (B, 1, H, W)).astype(F32)
    for k, v in enumerate((0.0, -0.0, 192.0, R.down(192.0), R.up(0.0), np.nan, np.inf)):
        disp.ravel()[k % disp.size] = v
    for k, v in enumerate((1.25, R.down(1.25), 0.0, -0.0, R.up(1.25), np.nan)):
        depth.ravel()[(k + 3) % depth.size] = v
    h, w = aux_hw
    one = np.dtype(dtype).type(1)
    below1 = np.nextafter(one, np.dtype(dtype).type(0))
    robot = np.where(rng.uniform(0, 1, (B, h, w)) > 0.35, rng.uniform(-0.999, 0.999, (B, h, w)), rng.uniform(1, 3, (B, h, w))).astype(dtype)
    specials = (below1, one, -0.5, -below1, -one, 0.0, -0.0, 2.5)
    for k, v in enumerate(specials):
        robot.ravel()[(5 * k + 1) % robot.size] = v
    rs = np.where(rng.uniform(0, 1, (B, h, w)) > 0.3, rng.uniform(0.2, 2.0, (B, h, w)), 0.0).astype(dtype)
    for k, v in enumerate((0.0, -0.0, np.finfo(dtype).tiny, -1.0, np.nan)):
        rs.ravel()[(3 * k + 2) % rs.size] = v
    return disp, depth, robot, rs
