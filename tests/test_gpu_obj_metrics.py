"""GPU: K22 az_obj_metrics -- the error metrics of a batch per image and per object label in one launch -- through the C ABI
and through ops.obj_metrics, cascade_metrics.compute_obj_err, compute_obj_err_per_image and compute_err_metric_per_image,
against the restatement and by the rules of tests/_obj_metrics_ref.py: counts, presence and stats exact, the two sums within
the reordering bound of fsum of their float32 terms, NaN / inf by class per (image, label).  Images of 1 ... 1000 pixels,
batches whose image boundaries fall inside what a flat index would call one block, one image past the grid cap; labels
constant, changing every pixel (64 in a wave), in runs that straddle waves and blocks, in blobs, and absent; both depth
sources; labels outside [0, L) and NaN pixels beside every special position (tests/test_obj_metrics_cpu.py shows which wrong
kernels fail here).

Measured on an MI355X (largest err / bound over all cases of this file, which prints them; every count, presence and stats
word equal): acc[0] 0 (|dg - dp| spans so few binades that fp64 adds the terms exactly), acc[3] 0.27 (the millimetre terms: the
allowance for the contracted multiply-add is what is used)."""
import math
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from activezero_amd import ops  # noqa: E402
from activezero_amd.ops import _call, _p, _stream  # noqa: E402
from activezero_amd.utils import cascade_metrics as cm  # noqa: E402
from tests import _obj_metrics_ref as O  # noqa: E402
from tests import _reduce_ref as R  # noqa: E402

DEV = torch.device("cuda", 0)
WORST = {}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    print("\n  largest err / bound per sum over this run: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(WORST.items())))


def upload(c):
    return {k: dev(c[k]) for k in ("dg", "zg", "dp", "zp", "fb", "mask", "label")}


def launch(out, d, c, explicit):
    acc, present, stats = out
    _call("az_obj_metrics", _p(acc), _p(present), _p(stats), _p(d["dg"]), _p(d["zg"]), _p(d["dp"]), _p(d["zp"]) if explicit else None,
          _p(d["fb"]), _p(d["mask"]), _p(d["label"]), c["B"], c["L"], c["per_batch"], _stream())


def outputs(c, acc_fill=0.0, int_fill=0):
    return (torch.full((c["B"], c["L"], 8), acc_fill, dtype=torch.float64, device=DEV),
            torch.full((c["B"], c["L"]), int_fill, dtype=torch.int32, device=DEV),
            torch.full((1,), int_fill, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("k", range(len(O.SHAPES)), ids=O.SHAPE_IDS)
def test_obj_metrics_per_cell(k, capsys):
    seen = 0
    for c, path, zp in O.cases(k):
        d = upload(c)
        out = outputs(c)
        launch(out, d, c, zp is not None)
        got = tuple(host(t) for t in out)
        info = O.check_k22(got, c, zp, what=f"az_obj_metrics {path}")
        for key, v in info.items():
            WORST[key] = max(WORST.get(key, 0.0), v)
        if c["label"] is None:  # exactly what az_disp_metrics is held to, image by image
            for b in range(c["B"]):
                R.check_k12_metrics(got[0][b, 0], *O.image_slice(c, zp, b), what=f"az_obj_metrics {c['name']} {path} image {b}")
        launch(out, d, c, zp is not None)  # the header promises +=
        O.check_k22(tuple(host(t) for t in out), c, zp, calls=2, what=f"az_obj_metrics {path}, two calls")
        # the wrapper: the same numbers, and nothing synchronises
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            res = ops.obj_metrics(d["dg"], d["zg"], d["dp"], d["mask"], d["label"], c["L"], d["fb"], d["zp"] if zp is not None else None)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        O.check_k22(tuple(host(t) for t in res), c, zp, what=f"ops.obj_metrics {path}")
        seen += 1
    with capsys.disabled():
        print(f"\n  az_obj_metrics {O.SHAPE_IDS[k]}: {seen} cases, " + ", ".join(f"{a} {v:.2e}" for a, v in sorted(WORST.items())), end="")
    assert seen == 2 * len(O.LAYOUTS)


def test_obj_metrics_adds_to_what_the_outputs_hold():
    """accumulators pre-filled with a sentinel: the call adds and never overwrites, and cells it has nothing for keep the
    sentinel to the bit.  A cell receives at most one atomic per workgroup of its image, each rounded at the size of
    sentinel + sum, hence the bound (blocks + 1) 2^-52 (sentinel + |sum|); counts stay exact integers"""
    base, ibase = 2.0 ** 20, 1000
    for c, path, zp in O.cases(8):  # 3 x 1 x 7 x 33
        d = upload(c)
        zero, filled = outputs(c), outputs(c, base, ibase)
        launch(zero, d, c, zp is not None)
        launch(filled, d, c, zp is not None)
        (a0, p0, s0), (a1, p1, s1) = (tuple(host(t) for t in o) for o in (zero, filled))
        assert np.array_equal(p1 - ibase, p0) and np.array_equal(s1 - ibase, s0)
        for slot in (1, 2, 4, 5, 6, 7):
            assert np.array_equal(a1[..., slot] - base, a0[..., slot])
        lim = (O.blocks_per_image(c["B"], c["per_batch"]) + 1) * 2.0 ** -52
        for slot in (0, 3):
            x0, x1 = a0[..., slot], a1[..., slot]
            fin = np.isfinite(x0)
            assert np.array_equal(np.isnan(x0), np.isnan(x1))
            assert (np.abs((x1 - base) - x0)[fin] <= lim * (base + np.abs(x0[fin]))).all()
            assert (x1[fin & (x0 == 0)] == base).all()


# ---- the wrappers -----------------------------------------------------------------------------------------------------
def clean_case(shape, seed, layout="blobs", L=17):
    """metrics_case with labels and no hostile pixel: what the drop-in functions are meant for"""
    c = dict(R.metrics_case(shape, seed))
    c.update(label=O.labels(layout, shape, L).reshape(shape), L=L, name=f"{c['name']} {layout}")
    return c


def wrapper_args(c, sl=slice(None)):
    d = upload(c)
    focal = d["fb"].reshape(-1, 1, 1, 1)
    return (d["dg"][sl], d["zg"][sl], d["dp"][sl], focal[sl], torch.ones_like(focal[sl])), d["label"][sl], d["mask"][sl].bool()


def test_compute_obj_err_against_the_golden_reference_output(golden):
    """g10 holds the reference's own compute_obj_err output (float32 means of 170 - 200 pixels: the tolerance of
    tests/test_gpu_loss_metrics.py::test_metrics_golden); the label arrives as the loader's float map"""
    g = golden("g10_metrics")
    gt, mask, zg, dp, focal, base, label = (dev(g[k]) for k in ("gt", "mask", "depth_gt", "disp_pred", "focal", "baseline", "label"))
    assert label.dtype == torch.float32
    for lab in (label, label.to(torch.int64), label.to(torch.int32), label.to(torch.uint8)):
        obj = cm.compute_obj_err(gt[:1], zg[:1], dp[:1], focal[:1], base[:1], lab, mask[:1])
        for i, o in enumerate(obj):
            assert o.shape == (17,) and o.dtype == np.float64
            np.testing.assert_allclose(o, g[f"obj{i}"], rtol=2e-6, atol=1e-9)


@pytest.mark.parametrize("shape", [R.SHAPED[1], (4, 1, 30, 50)], ids=["2x1x24x40", "4x1x30x50"])
def test_wrappers_against_the_loops_they_replace(shape):
    c = clean_case(shape, 8300)
    B, L = c["B"], c["L"]
    args, label, mask = wrapper_args(c)
    got = cm.compute_obj_err(*args, label, mask)
    # the per-object loop over ops.disp_metrics, as compute_obj_err ran before K22
    depth_pred = dev((c["fb"].reshape(-1, 1, 1, 1) / c["dp"]).astype(np.float32))  # IEEE float32 division, as the kernels'
    loop = {}
    for obj in label.unique().tolist():
        loop[int(obj)] = ops.disp_metrics(args[0], args[1], args[2], (label == obj) & mask, None, depth_pred).tolist()
    cells, present, _ = O.k22(c, None)
    assert sorted(loop) == sorted(np.flatnonzero(present.sum(axis=0)).tolist()) and len(loop) >= 10
    vals, lims, count = O.obj_err_scalars(c, None, per_image=False)
    assert np.array_equal(got[3], count)
    for l in range(L):
        if l not in loop:
            assert all(got[k][l] == 0 for k in range(4))
            continue
        r = O._merge([cells[b, l] for b in range(B)])
        n = r["counts"][5]
        assert loop[l][7] == n and n > 0 and loop[l][5] == r["counts"][3]  # counts equal
        assert got[2][l] == loop[l][5] / n
        # two fp64 sums of the same float32 terms in different orders: twice the reordering bound (and, for the millimetre
        # sum, twice the allowance for a contracted multiply-add, which the two kernels may or may not share)
        assert abs(got[0][l] - loop[l][0] / n) <= 2 * R.sum_bound(r["dd"]) / n + 4 * R.U * abs(got[0][l])
        assert abs(got[1][l] - loop[l][3] / n) <= 2 * (R.sum_bound(r["mm64"]) + R.fsum(r["mm_tol"])) / n + 4 * R.U * abs(got[1][l])
        for k in range(3):  # ... and against the fp64 formula on the exact accumulators
            assert abs(got[k][l] - vals[k, l]) <= lims[k, l], (k, l, got[k][l], vals[k, l], lims[k, l])

    # per image: test.py's loop over single images
    per = cm.compute_obj_err_per_image(*args, label, mask)
    single = [cm.compute_obj_err(*(a[b:b + 1] for a in args), label[b:b + 1], mask[b:b + 1]) for b in range(B)]
    vals, lims, count = O.obj_err_scalars(c, None, per_image=True)
    assert np.array_equal(per[3], count) and np.array_equal(per[3], sum(s[3] for s in single)) and count.max() == B
    for k in range(3):
        assert (np.abs(per[k] - vals[k]) <= lims[k]).all(), k
        assert (np.abs(per[k] - sum(s[k] for s in single)) <= 2 * lims[k]).all(), k
    for explicit in (False, True):
        zp = c["zp"] if explicit else None
        dicts = cm.compute_err_metric_per_image(*args, mask, depth_pred=dev(zp))
        assert len(dicts) == B
        for b in range(B):
            one = cm.compute_err_metric(*(a[b:b + 1] for a in args), mask[b:b + 1], depth_pred=dev(None if zp is None else zp[b:b + 1]))
            want = R.metrics_scalars(*O.image_slice(c, zp, b))
            assert sorted(dicts[b]) == sorted(R.METRIC_KEYS)
            for key, (v, lim) in want.items():
                assert abs(dicts[b][key] - v) <= lim and abs(one[key] - v) <= lim, (b, key, dicts[b][key], one[key], v, lim)


def test_compute_obj_err_is_one_launch_and_one_copy(monkeypatch):
    c = clean_case((2, 1, 24, 40), 8310)
    args, label, mask = wrapper_args(c)
    calls = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *a: (calls.append(name), real(name, *a)))
    torch.cuda.synchronize()
    for fn in (cm.compute_obj_err, cm.compute_obj_err_per_image):
        del calls[:]
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                fn(*args, label, mask)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        assert calls == ["az_obj_metrics"], calls
        syncs = [w for w in caught if "synchroniz" in str(w.message)]
        assert len(syncs) == 1, [str(w.message) for w in caught]
    torch.cuda.set_sync_debug_mode("error")  # ... and up to that copy nothing synchronises at all
    try:
        buf, b, nl = ops._obj_metrics(args[0], args[1], args[2], mask, label, 17, (args[3] * args[4]).reshape(-1), None)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert (b, nl) == (2, 17) and buf.numel() == ops._obj_words(2, 17)


@pytest.mark.parametrize("bad", [17, -1, 2 ** 31 - 1])
def test_a_label_outside_the_objects_raises_index_error(bad):
    c = clean_case((2, 1, 24, 40), 8320)
    c["label"].ravel()[1000] = bad
    c["mask"].ravel()[1000] = 0  # (masked or not)
    args, label, mask = wrapper_args(c)
    for fn in (cm.compute_obj_err, cm.compute_obj_err_per_image):
        with pytest.raises(IndexError, match="1 pixels"):
            fn(*args, label, mask)
    if bad == 17:
        assert cm.compute_obj_err(*args, label, mask, obj_total_num=18)[3][17] == 1


def test_an_object_that_is_present_but_fully_masked_gives_nan_with_count_one():
    c = clean_case((2, 1, 24, 40), 8330)
    hide = (c["label"] == 5) & (np.arange(2).reshape(2, 1, 1, 1) == 1)  # object 5 of image 1
    assert hide.sum() > 10
    c["mask"][hide] = 0
    args, label, mask = wrapper_args(c)
    per = cm.compute_obj_err_per_image(*args, label, mask)
    assert per[3][5] == 2 and all(math.isnan(per[k][5]) for k in range(3))  # image 0's mean + NaN
    assert np.isfinite(per[0][np.arange(17) != 5]).all()
    one = cm.compute_obj_err(*(a[1:] for a in args), label[1:], mask[1:])
    assert one[3][5] == 1 and all(math.isnan(one[k][5]) for k in range(3)) and np.isfinite(one[0][:5]).all()
    whole = cm.compute_obj_err(*args, label, mask)  # the batch as one set: image 0's pixels of the object remain
    assert whole[3][5] == 1 and np.isfinite(whole[0][5])
    dicts = cm.compute_err_metric_per_image(*args, torch.zeros_like(mask))
    assert all(math.isnan(v) for dct in dicts for v in dct.values())
