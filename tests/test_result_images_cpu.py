"""CPU side of the result images (K24, az_result_img.hip): the numpy restatement of tests/_result_images_ref.py against the
bytes matplotlib's plt.imsave wrote for the committed cases (tests/golden/g16_result_images.npz) and, where matplotlib is
installed, against the live call; the mutants the cases must tell from the right rule; the exported C entry point and its
host-side argument validation; the panel order; the PNG writer.  No kernel is launched."""
import ctypes
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

from activezero_amd import _lib, build
from tests import _gt_prep_ref as G
from tests import _result_images_ref as ref

ENULL, EINVAL = _lib.CONST["AZ_ENULL"], _lib.CONST["AZ_EINVAL"]
NAN, INF = float("nan"), float("inf")
CASES = ("one_on", "one_off", "batch3", "clip", "boundary", "md100", "contract", "pitched")
SAVE_IMG_DIRS = ("pred_disp", "gt_disp", "pred_disp_abs_err_cmap", "pred_depth", "gt_depth", "pred_depth_abs_err_cmap")


@pytest.fixture(scope="module")
def handle():
    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def cases():
    return ref.golden_cases()


def _tool():
    spec = importlib.util.spec_from_file_location("make_result_image_goldens", os.path.join(ref.REPO, "tools", "make_result_image_goldens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the restatement against matplotlib ------------------------------------------------------------------------------
def test_committed_cases_are_the_builders_cases(cases):
    built = ref.build_cases()
    assert tuple(cases) == tuple(built) == CASES
    for name, case in built.items():
        for k in ref.INPUTS:
            got = cases[name][0][k]
            assert got.dtype == np.asarray(case[k]).dtype and np.array_equal(got, case[k], equal_nan=got.dtype.kind == "f"), (name, k)
    assert os.path.getsize(ref.GOLDEN) < 200 * 1024


def test_cases_hold_what_they_are_for(cases):
    assert [cases[n][0]["mask"].reshape(-1).tolist() for n in ("one_on", "one_off")] == [[1], [0]]
    c = cases["batch3"][0]
    assert c["gt_disp"].shape == (3, 1, 12, 231) and 231 % 4 == 3 and len(set(zip(c["focal"].tolist(), c["baseline"].tolist()))) == 3
    pd, on = ref.pred_view(c), c["mask"] != 0
    assert on[0].all() and np.isnan(pd[0]).sum() == 1 and (pd[0] == 0).sum() == 1  # fully valid, a NaN, an infinite depth
    assert not on[1].all() and np.isnan(pd[1][on[1]]).sum() == 1 and not on[1, 0, :10, :220].all()  # masked pixels, under the legend too
    assert on[2].all() and (c["gt_disp"][2] == -1).sum() == 1 and (pd[2] == -1).sum() == 0 and np.isnan(pd[2]).sum() == 1
    assert ref.run_case(c)[1].tolist() == [0, 0b11011, 0b00010]  # the flags: per image and per panel
    assert cases["clip"][0]["gt_disp"].shape == (1, 1, 7, 53)
    b = cases["boundary"][0]
    row = b["gt_disp"][0, 0, 0]
    for j in (0, 1, 128, 255, 256):  # j * 0.75 and its two neighbours
        t = np.float32(0.75 * j)
        assert row[3 * j:3 * j + 3].tolist() == [np.nextafter(t, np.float32(-INF)), t, np.nextafter(t, np.float32(INF))]
        t = np.float32(j * 5 / 1024)
        assert b["gt_depth"][0, 0, 0, 3 * j + 1] == t and np.float32(np.float32(t / np.float32(1.25)) * np.float32(256)) == j
    tail = row[771:]
    assert tail[:2].tolist() == [0, 0] and np.signbit(tail[1]) and tail[2] == INF and tail[3] == -INF and 0 < tail[4] < np.finfo(np.float32).tiny
    pz = np.float32(ref.FOCAL * ref.BASELINE) / ref.pred_view(b)[0, 0, 1, :768]
    on_bound = (pz.reshape(256, 3) == (np.arange(1, 257, dtype=np.float32) * np.float32(5) / np.float32(1024))[:, None]).any(1)
    assert on_bound.sum() >= 128  # the predicted depth lands ON at least half of the bounds, and beside all of them
    q = cases["md100"][0]["gt_disp"].astype(np.float64) / 100.0
    assert cases["md100"][0]["max_disp"] == 100 and (q.astype(np.float32) != q).mean() > 0.9  # the quotient is inexact
    p = cases["pitched"][0]
    assert p["pred"].shape == (2, 1, 13, 35) and p["view"].tolist() == [4, 9, 30] and (p["pred"][:, :, :4] == 7777).all()


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_committed_imsave_bytes(cases, name):
    case, want = cases[name]
    got, _ = ref.run_case(case)
    assert got.dtype == np.uint8 and got.shape == want.shape == ref.pred_view(case).shape[:1] + (6,) + ref.pred_view(case).shape[2:] + (4,)
    assert np.array_equal(got, want), np.argwhere((got != want).any(-1))[:8]


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_live_imsave(cases, name):
    pytest.importorskip("matplotlib")
    pytest.importorskip("PIL")
    case, _ = cases[name]
    want = _tool().matplotlib_images(case)
    got, _ = ref.run_case(case)
    assert np.array_equal(got, want), np.argwhere((got != want).any(-1))[:8]


def test_table_header_is_the_committed_table_and_matplotlibs():
    tab = ref.table()
    assert tab.shape == (256, 4) and tab[0].tolist() == [68, 1, 84, 255] and tab[255].tolist() == [253, 231, 36, 255]
    assert np.array_equal(ref.header_table(), tab[:, :3])
    if importlib.util.find_spec("matplotlib") is not None:
        tool = _tool()
        live = tool.viridis_table()
        assert np.array_equal(live, tab[:, :3])
        with open(ref.HEADER) as f:
            assert f.read() == tool.header_text(live)


def test_imsave_returns_the_error_tables_integers():
    """(c * 255).astype(uint8) on K19's float32 k / 255 is k, for every value of the table"""
    ks = sorted({k for rgb in G.RGB for k in rgb})
    assert len(ks) == 29
    c = np.array(ks, np.float32) / np.float32(255.0)
    assert ((c * 255).astype(np.uint8)).tolist() == ks
    assert np.array_equal((G.colours() * 255).astype(np.uint8), np.array(G.RGB, np.uint8))


# ---- the mutants -------------------------------------------------------------------------------------------------------
KILLED_BY = {"recip": "boundary", "round": "batch3", "swap": "boundary", "bad_from_mask": "batch3", "nan_red": "batch3",
             "nan_first": "batch3", "one_flag": "batch3", "depth_assoc": "boundary", "fma": "contract", "fma_est": "contract",
             "legend_before_mask": "batch3", "alpha_from_mask": "one_off"}


@pytest.mark.parametrize("mutant", sorted(KILLED_BY))
def test_a_wrong_rule_changes_a_byte(cases, mutant):
    case, want = cases[KILLED_BY[mutant]]
    got, _ = ref.run_case(case, mutant=mutant)
    assert (got != want).any()


def test_every_contraction_pair_tells(cases):
    case, want = cases["contract"]
    for mutant in ("fma", "fma_est"):
        got, _ = ref.run_case(case, mutant=mutant)
        assert (got[0, 5, 10:] != want[0, 5, 10:]).any(-1).all()  # all 80 pairs land in another row


def test_the_256_step_cannot_be_seen():
    """The one rule of the list no case can test.  Colormap.__call__ sets xa == 256 to 255, i.e. table[255]; without the step
    the value is `over`, and the over colour of viridis IS table[255] (nobody calls set_over).  So leaving the step out changes
    no byte of any input -- shown here on the very values (192 and 1.25, where xa == 256) -- and the kernel keeps the step only
    because it is matplotlib's order."""
    assert set(KILLED_BY) | {"no_256"} == set(ref.MUTANTS)
    x = np.array([[[[192.0, np.nextafter(np.float32(192), np.float32(0)), np.nextafter(np.float32(192), np.float32(INF))]]]], np.float32)
    z = np.float32(ref.FOCAL * ref.BASELINE) / x
    args = (x, x, z, np.ones(x.shape, bool), [ref.FOCAL], [ref.BASELINE], 192.0)
    plain, mutant = ref.result_images(*args)[0], ref.result_images(*args, mutant="no_256")[0]
    assert np.array_equal(plain, mutant)
    assert plain[0, 0, 0].tolist() == [ref.table()[255].tolist(), ref.table()[255].tolist(), ref.table()[255].tolist()]
    if importlib.util.find_spec("matplotlib") is not None:
        import matplotlib.pyplot as plt

        cmap = plt.get_cmap("viridis")
        assert cmap(np.float32(1.0), bytes=True) == cmap(np.float32(1.5), bytes=True) == tuple(ref.table()[255])


# ---- the C surface -----------------------------------------------------------------------------------------------------
def test_entry_point_is_exported_and_typed(handle):
    assert "az_result_images" in _lib.declared_symbols()
    P, I, L, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
    assert _lib._SIGS["az_result_images"] == [P, P, P, L, L, P, P, P, P] + [Fl] * 6 + [I] * 3 + [P]
    assert handle.az_result_images.argtypes == _lib._SIGS["az_result_images"] and handle.az_result_images.restype is I
    assert _lib.expected_abi_version() == 6 and handle.az_abi_version() == 6  # the entry point was only added


def test_entry_point_rejects_before_any_launch(handle):
    """every call below must be refused on the host: there is no device here"""
    buf = (ctypes.c_float * 16)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    f = handle.az_result_images

    def call(out=p, flags=p, pred=p, row_stride=231, img_stride=12 * 231, gt_disp=p, gt_depth=p, mask=p, fb=p, max_disp=192.0,
             depth_hi=1.25, b=1, h=12, w=231):
        return f(out, flags, pred, row_stride, img_stride, gt_disp, gt_depth, mask, fb, max_disp, depth_hi, 3.0, 0.05, 1000.0, 1.0,
                 b, h, w, None)

    for hole in ("out", "flags", "pred", "gt_disp", "gt_depth", "mask", "fb"):
        assert call(**{hole: None}) == ENULL, hole
    for name in ("b", "h", "w"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -3}) == EINVAL
    assert call(row_stride=230) == EINVAL and call(row_stride=0) == EINVAL and call(row_stride=-231) == EINVAL
    assert call(img_stride=-1) == EINVAL
    for bad in (0.0, -192.0, NAN):
        assert call(max_disp=bad) == EINVAL and call(depth_hi=bad) == EINVAL
    assert call(out=ctypes.c_void_p(ctypes.addressof(buf) + 2)) == EINVAL  # a pixel is one 4-byte word


# ---- the Python surface ----------------------------------------------------------------------------------------------
def test_panel_order_is_save_imgs():
    from activezero_amd import ops
    from activezero_amd.utils import result_images as ri

    assert ops.RESULT_PANELS == ri.PANELS == ref.PANELS == SAVE_IMG_DIRS
    # ... and the restatement's panels are those maps: viridis of the four maps, the two error images
    case, want = ref.golden_cases()["clip"]
    on = case["mask"][0, 0] != 0
    below = np.ones_like(on)
    below[:10, :220] = False  # outside the legend
    pz = np.float32(case["focal"][0] * case["baseline"][0]) / ref.pred_view(case)
    for m, kind, est, gt in ((2, "disp", ref.pred_view(case), case["gt_disp"]),
                             (5, "depth", pz * np.float32(1000), case["gt_depth"] * np.float32(1000))):
        img = (G.error_img(est[:, 0], gt[:, 0], on[None], kind)[0] * 255).astype(np.uint8)
        assert np.array_equal(want[0, m, :, :, :3], img) and (want[0, m, :, :, 3] == 255).all()
    for m in ref.VIRIDIS_PANELS:
        assert (want[0, m][~on] == ref.RED).all() and not (want[0, m][on] == ref.RED).all(-1).any()
    assert not np.array_equal(want[0, 0], want[0, 1]) and not np.array_equal(want[0, 3], want[0, 4])


def test_signatures():
    from activezero_amd import ops
    from activezero_amd.utils import result_images as ri

    def params(fn):
        return [(n, q.default) for n, q in inspect.signature(fn).parameters.items()]

    none = inspect.Parameter.empty
    assert params(ops.result_images)[:11] == [("pred_disp", none), ("gt_disp", none), ("gt_depth", none), ("mask", none),
                                              ("focal_x_baseline", none), ("max_disp", none), ("depth_hi", 1.25),
                                              ("disp_abs_thres", 3.0), ("disp_rel_thres", 0.05), ("depth_scale", 1000.0),
                                              ("depth_abs_thres", 1.0)]
    assert [n for n, _ in params(ri.render_result_images)][:7] == ["pred_disp", "img_disp_l", "img_depth_l", "mask", "focal_length",
                                                                  "baseline", "max_disp"]
    assert [n for n, _ in params(ri.save_result_images)] == ["log_dir", "prefixes", "images"]


def test_python_surface_refuses_cpu_tensors_and_wrong_shapes():
    from activezero_amd import ops

    d = torch.zeros(2, 1, 8, 12)
    fb = torch.ones(2)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.result_images(d, d, d, d > 0, fb, 192)
    with pytest.raises(RuntimeError, match=r"\[B,1,H,W\]"):
        ops.result_images(d[:, 0], d, d, d > 0, fb, 192)
    with pytest.raises(RuntimeError, match="stride 1"):
        ops.result_images(torch.zeros(2, 1, 12, 8).transpose(2, 3), d, d, d > 0, fb, 192)


def test_save_result_images_round_trips(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from activezero_amd.utils import result_images as ri

    rng = np.random.default_rng(2408)
    images = rng.integers(0, 256, (2, 6, 7, 13, 4), dtype=np.uint8)  # alpha too: the decoded pixels are the contract
    paths = ri.save_result_images(str(tmp_path), ["0-300002", "1-300135"], images)
    assert len(paths) == 12 == len(set(paths))
    for b, prefix in enumerate(("0-300002", "1-300135")):
        for m, panel in enumerate(SAVE_IMG_DIRS):
            path = os.path.join(str(tmp_path), panel, prefix + ".png")
            assert path in paths
            with Image.open(path) as im:
                assert im.mode == "RGBA" and np.array_equal(np.array(im), images[b, m])
    with pytest.raises(RuntimeError, match="prefixes"):
        ri.save_result_images(str(tmp_path), ["a"], images)
    with pytest.raises(RuntimeError, match="uint8"):
        ri.save_result_images(str(tmp_path), ["a", "b"], images.astype(np.float32))
