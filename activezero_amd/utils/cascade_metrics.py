"""Error metrics -- drop-in for the reference's utils/cascade_metrics.py:16-62
(`compute_err_metric`): same arguments, same dict of Python floats, computed in one pass by the
K12 kernel (az_disp_metrics) and fetched with a single device->host copy instead of ten masked
reductions with an .item() each.  `compute_obj_err` (cascade_metrics.py:65-126, imported by
test.py) is one pass of the K22 kernel (az_obj_metrics) for all objects -- no label.unique(), no
per-object temporaries -- and one copy.  `compute_obj_err_per_image` and
`compute_err_metric_per_image` are additions: the numbers test.py gets by looping over the images
of a batch one at a time, from one launch and one copy for the whole batch.
"""
import numpy as np
import torch

from activezero_amd import ops

_KEYS = ("epe", "bad1", "bad2", "depth_abs_err", "depth_err2", "depth_err4", "depth_err8")


def _depth_source(disp_gt, disp_pred, focal_length, baseline, depth_pred):
    """(focal_x_baseline [bs] or None, depth_pred or None): one value per image where the arguments allow it"""
    if depth_pred is not None:
        return None, depth_pred
    fb = (focal_length * baseline).to(torch.float32)
    bs = disp_gt.shape[0]
    if fb.numel() == 1:
        fb = fb.reshape(1).expand(bs)
    if fb.numel() != bs:  # a full map: materialise depth_pred as the reference does
        return None, fb / disp_pred
    return fb, None


def _err_dict(acc):
    n = acc[7]
    div = (lambda v: v / n) if n > 0 else (lambda v: float("nan"))
    return {k: div(acc[i]) for i, k in enumerate(_KEYS)}


@torch.no_grad()
def compute_err_metric(disp_gt, depth_gt, disp_pred, focal_length, baseline, mask, depth_pred=None):
    """disp_gt, depth_gt, disp_pred [bs,1,H,W]; focal_length, baseline broadcastable per batch element
    (the dataset yields [bs,1,1,1], datasets/messytable.py:286-297); mask bool [bs,1,H,W]."""
    fb, depth_pred = _depth_source(disp_gt, disp_pred, focal_length, baseline, depth_pred)
    return _err_dict(ops.disp_metrics(disp_gt, depth_gt, disp_pred, mask, fb, depth_pred).tolist())


@torch.no_grad()
def compute_err_metric_per_image(disp_gt, depth_gt, disp_pred, focal_length, baseline, mask, depth_pred=None):
    """compute_err_metric of every image of the batch on its own: a list of bs dicts of the seven keys, from one launch
    (az_obj_metrics without labels) and one device->host copy."""
    fb, depth_pred = _depth_source(disp_gt, disp_pred, focal_length, baseline, depth_pred)
    acc, _, _ = ops.obj_metrics_host(disp_gt, depth_gt, disp_pred, mask, None, 1, fb, depth_pred)
    return [_err_dict(row) for row in acc[:, 0].tolist()]


def _label_i32(label):
    """integer labels of any width are cast to int32, float labels truncated (the loader's are integral; test.py casts them)"""
    return label if label.dtype == torch.int32 else label.to(torch.int32)


def _obj_tables(disp_gt, depth_gt, disp_pred, focal_length, baseline, label, mask, obj_total_num):
    """acc [bs,L,8], present [bs,L] on the host; IndexError for a label outside [0, obj_total_num)"""
    fb, depth_pred = _depth_source(disp_gt, disp_pred, focal_length, baseline, None)
    mask = mask if mask.dtype in (torch.bool, torch.uint8) else mask.bool()
    acc, present, stats = ops.obj_metrics_host(disp_gt, depth_gt, disp_pred, mask, _label_i32(label), obj_total_num, fb,
                                               depth_pred)
    if stats[0]:
        raise IndexError(f"{int(stats[0])} pixels carry an object label outside [0, {obj_total_num})")
    return acc, present


def _obj_means(acc, present, out):
    """out[k][l] += the mean of object l (NaN when every pixel of it is masked), count += 1, for the objects present"""
    disp_err, depth_err, depth_4_err, count = out
    for l in np.flatnonzero(present):
        n = acc[l, 7]
        disp_err[l] += acc[l, 0] / n if n else float("nan")
        depth_err[l] += acc[l, 3] / n if n else float("nan")
        depth_4_err[l] += acc[l, 5] / n if n else float("nan")
        count[l] += 1


@torch.no_grad()
def compute_obj_err(disp_gt, depth_gt, disp_pred, focal_length, baseline, label, mask, obj_total_num=17):
    """Per-object disparity / depth errors (cascade_metrics.py:65-126): returns
    (total_obj_disp_err, total_obj_depth_err, total_obj_depth_4_err, total_obj_count), numpy [obj_total_num].
    One launch and one device->host copy for any number of objects.  The whole batch is one set of pixels, as in the
    reference (which calls it with one image).  An object that is present but fully masked gives NaN with count 1 (the
    reference divides by zero there).  A label >= obj_total_num raises IndexError, as the reference's indexing does; so
    does a negative one -- the reference lets -1 wrap round to the last object through numpy indexing, an accident that is
    not reproduced."""
    acc, present = _obj_tables(disp_gt, depth_gt, disp_pred, focal_length, baseline, label, mask, obj_total_num)
    out = tuple(np.zeros(obj_total_num) for _ in range(4))
    _obj_means(acc.sum(axis=0), present.sum(axis=0), out)
    return out


@torch.no_grad()
def compute_obj_err_per_image(disp_gt, depth_gt, disp_pred, focal_length, baseline, label, mask, obj_total_num=17):
    """What test.py accumulates by calling compute_obj_err on the images of the batch one at a time: per object the sum
    over the images of that image's mean, and the number of images the object appears in -- from one launch and one copy."""
    acc, present = _obj_tables(disp_gt, depth_gt, disp_pred, focal_length, baseline, label, mask, obj_total_num)
    out = tuple(np.zeros(obj_total_num) for _ in range(4))
    for b in range(acc.shape[0]):
        _obj_means(acc[b], present[b], out)
    return out
