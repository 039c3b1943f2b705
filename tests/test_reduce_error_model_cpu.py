"""CPU: the checks of tests/test_gpu_reduce_exact.py bite.  tests/_reduce_ref.py restates the loss, metric and amax
reductions per pixel in float32 and states the rules a GPU result is held to; here
  * the restatement agrees with torch's own fp64 autograd for both losses, forward and backward, and with
    oracle/metrics_oracle.py for the metrics;
  * the launch caps the map sizes are built around are still in the sources;
  * the restatement passes its own rules on every case, and each of the wrong kernels listed in MUTANTS -- a deliberately
    wrong copy of the restatement playing the kernel -- is rejected by the rules on at least one case, which is named;
  * az_absmax_multi is in the C ABI, validates on the host, and its descriptor table holds the bytes of the struct."""
import ctypes
import math
import os
import re
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from activezero_amd import _lib, amax, build
from oracle import metrics_oracle as mo
from tests import _reduce_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "activezero_amd", "csrc")
T = torch.from_numpy
F32 = np.float32
_CASES = {}


def cases(kind, **kw):
    """the cases of one input family, smallest maps first, built once"""
    key = (kind, tuple(sorted(kw.items())))
    if key not in _CASES:
        make, seed = {"loss": (R.loss_case, 7200), "metrics": (R.metrics_case, 7300), "seq": (R.seq_case, 7400)}[kind]
        _CASES[key] = list(R.map_cases(make, seed, **kw))
    return _CASES[key]


# ---- the restatement against torch's own arithmetic ---------------------------------------------------------------------------
def test_disp_loss_restatement_agrees_with_fp64_autograd():
    c = R.loss_case((3, 1, 7, 33), 7201)
    for mode, mask, lo, hi in R.loss_modes(c):
        gt = T(c["gt"]).double()
        ok = T(c["mask"] != 0) if mask is not None else (gt > lo) & (gt < hi)
        ps = [T(p).double().requires_grad_() for p in c["preds"]]
        loss = sum(w * F.smooth_l1_loss(p[ok], gt[ok], reduction="mean") for w, p in zip(R.LOSS_WEIGHTS, ps))
        (loss * 1.75).backward()
        want, bound = R.disp_loss_scalar(c["preds"], c["gt"], mask, lo, hi)
        terms, count = R.k12_fwd(c["preds"], c["gt"], mask, lo, hi)
        assert count == int(ok.sum()) and count > 100, mode
        # float32 terms: |p - g| and the branch's two operations, one rounding each
        assert abs(want - loss.item()) <= 4 * 2.0 ** -24 * abs(loss.item()), mode
        got = R.k12_bwd(c["preds"], c["gt"], mask, lo, hi, 1.75, count)
        for g, p in zip(got, ps):  # subtraction, division by the count, w * s, the product: four roundings
            np.testing.assert_allclose(g, p.grad.numpy(), rtol=4 * 2.0 ** -24, atol=0, err_msg=mode)
            assert np.array_equal(g == 0, p.grad.numpy() == 0), mode


@pytest.mark.parametrize("tsign", [1, -1])
@pytest.mark.parametrize("vkey", ["valid_f32", "valid_u8", "valid_bool"])
def test_sequence_loss_restatement_agrees_with_fp64_autograd(tsign, vkey):
    c = R.seq_case((3, 1, 7, 33), 7401)
    gt = T(c["gt"]).double()
    ok = (T(c[vkey].astype(np.float32)) >= 0.5) & (gt.abs() < R.MAX_FLOW)
    weights = (0.9, 1.0)
    ps = [T(p).double().requires_grad_() for p in c["preds"](tsign)]
    loss = sum(w * (p - tsign * gt).abs()[ok].mean() for w, p in zip(weights, ps))
    (loss * 0.5).backward()
    want, _ = R.seq_loss_scalar(c["preds"](tsign), c["gt"], c[vkey], R.MAX_FLOW, tsign, weights)
    assert abs(want - loss.item()) <= 2 * 2.0 ** -24 * abs(loss.item())
    for w, p, p32 in zip(weights, ps, c["preds"](tsign)):
        terms, count, bad = R.k16_fwd(p32, c["gt"], c[vkey], R.MAX_FLOW, tsign)
        assert count == int(ok.sum()) and bad == int((~torch.isfinite(T(p32))).sum()) and bad >= 3
        g = R.k16_bwd(p32, c["gt"], c[vkey], R.MAX_FLOW, tsign, 0.5, count, w)
        ref = p.grad.numpy()
        fin = np.isfinite(ref)  # (a NaN prediction on an invalid pixel: autograd's 0 * NaN; the kernel writes 0 there)
        np.testing.assert_allclose(g[fin], ref[fin], rtol=3 * 2.0 ** -24, atol=0)
        assert np.array_equal(g[fin] == 0, ref[fin] == 0) and not np.isnan(g[~fin]).any() and (g[~fin] == 0).all()


@pytest.mark.parametrize("explicit", [False, True])
def test_metrics_restatement_agrees_with_the_oracle(explicit):
    c = R.metrics_case((3, 1, 7, 33), 7301)
    mask = T(c["mask"] != 0)
    fb = T(c["fb"]).reshape(-1, 1, 1, 1)
    want = mo.compute_err_metric(T(c["dg"]), T(c["zg"]), T(c["dp"]), fb, torch.ones_like(fb), mask,
                                 depth_pred=T(c["zp"]) if explicit else None)
    have = R.metrics_scalars(c["dg"], c["zg"], c["dp"], c["zp"] if explicit else None, c["fb"], c["mask"], c["per_batch"])
    for k in ("bad1", "bad2", "depth_err2", "depth_err4", "depth_err8"):  # float32 comparisons on both sides: the same counts
        assert have[k][0] == want[k], k
    for k in ("epe", "depth_abs_err"):  # the oracle's float32 mean
        assert abs(have[k][0] - want[k]) <= 1e-5 * abs(want[k]) + have[k][1], k


# ---- the caps in the sources --------------------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_launch_caps_are_still_in_the_sources():
    common, dl, cu, ab = _src("az_common.h"), _src("az_disp_loss.hip"), _src("az_convex_up.hip"), _src("az_absmax.hip")
    grid_for = common[common.index("static inline unsigned az_grid_for("):]
    grid_for = grid_for[:grid_for.index("\n}")]
    assert "if (g > 256LL * 16) g = 256LL * 16;" in grid_for and 256 * 16 == R.EW_CAP
    for text, fn in ((dl, "dl_reduce_grid"), (cu, "sl_reduce_grid")):
        body = text[text.index(f"static unsigned {fn}("):]
        body = body[:body.index("\n}")]
        assert "return g > 1024u ? 1024u : g;" in body and R.RED_CAP == 1024, fn
    assert "#define DL_BLOCK 256" in dl and "#define SL_BLOCK 256" in cu and R.BLOCK == 256
    # which launch takes which grid
    assert len(re.findall(r"dim3\(dl_reduce_grid\(n\)\)", dl)) == 2 and len(re.findall(r"dim3\(az_grid_for\(n, DL_BLOCK\)\)", dl)) == 1
    assert len(re.findall(r"dim3\(sl_reduce_grid\(n\)\)", cu)) == 2 and len(re.findall(r"dim3\(az_grid_for\(n, SL_BLOCK\)\)", cu)) == 2
    assert "const long long n4 = n >> 2;" in ab and "dim3(az_grid_for((n + 3) / 4, 256))" in ab and R.ABSMAX_VEC == 4
    assert "threadIdx.x < (n & 3)" in ab
    assert (R.AMAX_SLOTS, R.AMAX_STRIDE, R.AMAX_FLOATS) == tuple(_lib.CONST[k] for k in ("AZ_AMAX_SLOTS", "AZ_AMAX_STRIDE", "AZ_AMAX_FLOATS"))
    assert R.N_RED == 262437 and R.N_EW == 1048869 and R.ABSMAX_N[-1] == 4195507
    assert 4 * R.ABSMAX_N[-1] <= 16 * 2 ** 20 + 2 ** 16  # the largest map: 16 MB


# ---- mutants ------------------------------------------------------------------------------------------------------------------
def _loss_fwd(defect):
    for c in cases("loss"):
        for mode, mask, lo, hi in R.loss_modes(c):
            yield (f"az_disp_loss_fwd {c['name']} {mode}", lambda: R.k12_fwd_acc(c["preds"], c["gt"], mask, lo, hi, defect),
                   lambda got: R.check_k12_fwd(got, c["preds"], c["gt"], mask, lo, hi))


def _loss_bwd(defect):
    for c in cases("loss", nonfinite_preds=True):
        for mode, mask, lo, hi in R.loss_modes(c):
            count = R.k12_fwd(c["preds"], c["gt"], mask, lo, hi)[1]
            yield (f"az_disp_loss_bwd {c['name']} {mode}",
                   lambda: R.k12_bwd(c["preds"], c["gt"], mask, lo, hi, 1.75, count, defect=defect),
                   lambda got: R.check_k12_bwd(got, c["preds"], c["gt"], mask, lo, hi, 1.75, count))


def _metrics(defect):
    for c in cases("metrics"):
        for path, zp in (("fb", None), ("depth_pred", c["zp"])):
            args = (c["dg"], c["zg"], c["dp"], zp, c["fb"], c["mask"], c["per_batch"])
            yield (f"az_disp_metrics {c['name']} {path}", lambda: R.k12_metrics_acc(*args, defect=defect),
                   lambda got: R.check_k12_metrics(got, *args))


def _seq_fwd(defect):
    for c in cases("seq"):
        for vkey in ("valid_f32", "valid_u8", "valid_bool"):
            for tsign in (1, -1):
                args = (c["preds"](tsign)[0], c["gt"], c[vkey], R.MAX_FLOW, tsign)
                yield (f"az_seq_loss_fwd {c['name']} {vkey} tsign={tsign}", lambda: R.k16_fwd_acc(*args, defect=defect),
                       lambda got: R.check_k16_fwd(got, *args))


def _seq_bwd(defect):
    for c in cases("seq", nonfinite_preds=True):
        for vkey in ("valid_f32", "valid_u8"):
            for tsign in (1, -1):
                pred = c["preds"](tsign)[1]
                count = R.k16_fwd(pred, c["gt"], c[vkey], R.MAX_FLOW, tsign)[1]
                args = (pred, c["gt"], c[vkey], R.MAX_FLOW, tsign, 0.5, count, 0.9)
                yield (f"az_seq_loss_bwd {c['name']} {vkey} tsign={tsign}", lambda: R.k16_bwd(*args, defect=defect),
                       lambda got: R.check_k16_bwd(got, *args))


def _absmax(defect):
    for n in R.ABSMAX_N:
        for name, x in R.absmax_cases(n):
            read = defect if defect == "slot0" else None
            kernel = None if defect == "slot0" else defect
            yield (f"az_absmax {name}", lambda: R.absmax_array(x, kernel), lambda got: R.check_absmax(got, x, defect=read))


MUTANTS = [  # (what is wrong, the runs it is tried on, the defect of tests/_reduce_ref.py)
    ("the last n % 256 elements are skipped (az_disp_loss_fwd)", _loss_fwd, "tail"),
    ("the last n % 256 elements are skipped (az_disp_loss_bwd)", _loss_bwd, "tail"),
    ("the last n % 256 elements are skipped (az_disp_metrics)", _metrics, "tail"),
    ("the last n % 256 elements are skipped (az_seq_loss_fwd)", _seq_fwd, "tail"),
    ("the last n % 256 elements are skipped (az_seq_loss_bwd)", _seq_bwd, "tail"),
    ("the stride loop stops after its first pass, reduction cap (az_disp_loss_fwd)", _loss_fwd, "one_pass"),
    ("the stride loop stops after its first pass, reduction cap (az_disp_metrics)", _metrics, "one_pass"),
    ("the stride loop stops after its first pass, reduction cap (az_seq_loss_fwd)", _seq_fwd, "one_pass"),
    ("the stride loop stops after its first pass, element-wise cap (az_disp_loss_bwd)", _loss_bwd, "one_pass"),
    ("the stride loop stops after its first pass, element-wise cap (az_seq_loss_bwd)", _seq_bwd, "one_pass"),
    ("dd >= 1 for dd > 1", _metrics, "ge0"),
    ("dd >= 2 for dd > 2", _metrics, "ge1"),
    ("dz >= 2e-3 for dz > 2e-3", _metrics, "ge2"),
    ("dz >= 4e-3 for dz > 4e-3", _metrics, "ge3"),
    ("dz >= 8e-3 for dz > 8e-3", _metrics, "ge4"),
    ("gt >= lo for gt > lo", _loss_fwd, "lo_incl"),
    ("gt <= hi for gt < hi", _loss_fwd, "hi_incl"),
    ("fb[0] for every batch element", _metrics, "fb0"),
    ("fb[(i + 255) / per_batch]: the block's index for the pixel's", _metrics, "fb_block"),
    ("mask byte == 1 for != 0 (az_disp_loss_fwd)", _loss_fwd, "mask_eq1"),
    ("mask byte == 1 for != 0 (az_disp_metrics)", _metrics, "mask_eq1"),
    ("a gradient clamp through fmin / fmax that drops NaN", _loss_bwd, "clamp_fmin"),
    ("sign(0) = 1 in K16", _seq_bwd, "sign0"),
    ("K16 validity > 0.5", _seq_fwd, "valid_gt"),
    ("K16 |gt| <= max_flow", _seq_fwd, "flow_le"),
    ("the non-finite counter restricted to valid pixels", _seq_fwd, "nonfinite_valid"),
    ("absmax ignores the n & 3 tail", _absmax, "no_tail"),
    ("absmax compares signed values", _absmax, "signed"),
    ("absmax keeps inf", _absmax, "keep_inf"),
    ("absmax reads only slot 0", _absmax, "slot0"),
]


@pytest.mark.parametrize("runs", [_loss_fwd, _loss_bwd, _metrics, _seq_fwd, _seq_bwd, _absmax], ids=lambda f: f.__name__[1:])
def test_the_restatement_passes_its_own_rules_on_every_case(runs):
    n = 0
    for name, kernel, rule in runs(None):
        rule(kernel())
        n += 1
    assert n >= 24


@pytest.mark.parametrize("what,runs,defect", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_every_mutant_is_rejected_by_the_rules(what, runs, defect, capsys):
    tried = 0
    for name, kernel, rule in runs(defect):
        tried += 1
        try:
            rule(kernel())
        except AssertionError as err:
            with capsys.disabled():
                print(f"\n  mutant '{what}' rejected by case {tried}: {name}\n    {err}", end="")
            return
    pytest.fail(f"mutant '{what}' survived all {tried} cases: a case is missing")


def test_the_smooth_l1_branch_at_d_le_1_is_no_defect():
    """`d <= 1` for `d < 1` is not a wrong kernel: the two branches meet at d = 1, (0.5f * 1) * 1 = 1 - 0.5f = 0.5 exactly, and
    nowhere else do the two conditions differ (a NaN takes the linear branch under both).  No input can tell them apart, at
    1 or beside it -- checked here at 1, at its float32 neighbours and on every case -- so no rule is asked to reject it;
    a branch point that is really misplaced, `d < 2`, is rejected."""
    d = np.array([R.down(1), 1, R.up(1), np.nan, 0, np.inf], dtype=F32)
    a, b = R.smooth_l1(d), R.smooth_l1(d, "branch_le")
    assert np.array_equal(a, b, equal_nan=True) and a[1] == F32(0.5)
    assert a[0] == F32(0.5) * R.down(1) * R.down(1) and a[2] == R.up(1) - F32(0.5) and a[0] < a[1] < a[2]
    for name, kernel, rule in _loss_fwd("branch_le"):
        rule(kernel())
    c = cases("loss")[8]
    wrong = [np.where(np.abs(p - c["gt"]) < 2, (F32(0.5) * np.abs(p - c["gt"])) * np.abs(p - c["gt"]), np.abs(p - c["gt"]) - F32(0.5))
             for p in c["preds"]]
    ok = c["mask"] != 0
    acc = np.array([R.fsum(w[ok]) for w in wrong] + [float(ok.sum())])
    with pytest.raises(AssertionError, match="acc4"):
        R.check_k12_fwd(acc, c["preds"], c["gt"], c["mask"], 0.0, math.inf)


def test_the_special_pixels_sit_where_kernels_go_wrong():
    for n, pb, want in ((1, 1, [0]), (257, 257, [0, 256]), (693, 231, [0, 230, 231, 461, 462, 692]),
                        (R.N_RED, R.N_RED, [0, 262143, 262144, R.N_RED - 1]),
                        (R.N_EW, R.N_EW, [0, 262143, 262144, 1048575, 1048576, R.N_EW - 1])):
        assert R.special_positions(n, pb) == want
    c = cases("loss")[-1]
    for i in R.special_positions(c["n"], c["per_batch"]):  # valid under the mask and under both ranges
        assert c["mask"].ravel()[i] != 0 and 1.0 < c["gt"].ravel()[i] < 192.0
    m = cases("metrics")[8]
    assert m["B"] == 3 and len(set(m["fb"].tolist())) == 3 and all(m["mask"].ravel()[i] != 0 for i in (230, 231, 461, 462))
    for c in cases("loss") + cases("metrics") + cases("seq"):  # free of subnormals except where stated
        for k in ("gt", "dg", "dp", "zg", "zp"):
            if k in c:
                v = np.abs(c[k][np.isfinite(c[k])])
                assert set(v[(v > 0) & (v < 2.0 ** -126)].tolist()) <= {float(F32(1e-45))}


# ---- az_absmax_multi in the C ABI ---------------------------------------------------------------------------------------------
def test_absmax_multi_is_declared_exported_and_validates_on_the_host():
    build.build()
    handle = _lib.lib()
    assert "az_absmax_multi" in _lib.declared_symbols() and hasattr(handle, "az_absmax_multi")
    assert _lib.expected_abi_version() == 6 and handle.az_abi_version() == 6  # additive change
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert handle.az_absmax_multi(None, p, p, 1, 1, None) == _lib.CONST["AZ_ENULL"]
    assert handle.az_absmax_multi(p, None, p, 1, 1, None) == _lib.CONST["AZ_ENULL"]
    assert handle.az_absmax_multi(p, p, None, 1, 1, None) == _lib.CONST["AZ_ENULL"]
    assert handle.az_absmax_multi(p, p, p, 0, 1, None) == _lib.CONST["AZ_EINVAL"]
    assert handle.az_absmax_multi(p, p, p, 1, 0, None) == _lib.CONST["AZ_EINVAL"]
    big = (ctypes.c_float * 16)()
    misaligned = ctypes.c_void_p(((ctypes.addressof(big) + 15) & ~15) + 4)
    assert handle.az_absmax(p, misaligned, 4, None) == _lib.CONST["AZ_EINVAL"]  # the alignment rule, before any launch
    assert handle.az_absmax(p, p, 0, None) == _lib.CONST["AZ_EINVAL"]


def test_absmax_table_bytes_are_the_struct_in_header_order():
    rows = [dict(src=0x7F0000001000, amax=0x7F0000002000, n=1), dict(src=0x7E0000000004, amax=0x7E0000003000, n=257),
            dict(src=0x10, amax=0x20, n=(1 << 20) + 1)]
    descs, block_desc, first, nblocks = amax.absmax_tables(rows)
    assert _lib.ABSMAX_DESC.itemsize == 24
    assert descs.view(np.uint8).tobytes() == b"".join(struct.pack("<QQq", r["src"], r["amax"], r["n"]) for r in rows)
    assert first.tolist() == [0, 1, 3] and nblocks == 3 + (1 << 12) + 1 and block_desc[:4].tolist() == [0, 1, 1, 2]
    assert block_desc.dtype == first.dtype == np.int32
    with pytest.raises(KeyError):
        amax.absmax_tables([dict(src=1, amax=2)])
