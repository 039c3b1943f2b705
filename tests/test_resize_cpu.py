"""CPU side of the real domain's resize (K21, az_resample.hip): the numpy restatement tests/_resize_ref.py against Pillow's
recorded outputs (tests/golden/g15_pil_resize.npz) and, where Pillow is installed, against Pillow itself; the library's
host-side coefficient tables against the restatement's, entry for entry; the exported C entry points with their
argument validation; and the refusals of the Python surface.  No kernel is launched."""
import ctypes
import os

import numpy as np
import pytest
import torch

from activezero_amd import _lib, build
from tests import _resize_ref as ref

NEW = ("az_resample_bilinear_ksize", "az_resample_bilinear_table", "az_resize_bilinear_u8")
EINVAL, EUNSUP = -1, -4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_pil_resize.npz")
PAIRS = ((8, 6), (3, 5), (720, 540), (1280, 960), (540, 540), (1, 4), (13, 1), (64, 8), (200, 25))
# first, count, then the non-zero coefficients: Pillow's answers
T_8_6 = ((0, 2, 2936013, 1258291), (1, 2, 2097152, 2097152), (2, 3, 1143901, 2669103, 381300),
         (3, 3, 381300, 2669103, 1143901), (5, 2, 2097152, 2097152), (6, 2, 1258291, 2936013))
T_3_5 = ((0, 1, 4194304), (0, 2, 2516582, 1677722), (1, 2, 4194304), (1, 2, 1677722, 2516582), (2, 1, 4194304))


@pytest.fixture(scope="module")
def handle():
    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _literal(rows, ks):
    out = np.zeros((len(rows), 2 + ks), np.int32)
    for i, row in enumerate(rows):
        out[i, :len(row)] = row
    return out


# ---- the restatement against Pillow ----------------------------------------------------------------------------------------
def test_restatement_reproduces_the_literal_tables():
    assert ref.ksize(8, 6) == 5 and np.array_equal(ref.table(8, 6), _literal(T_8_6, 5))
    assert ref.ksize(3, 5) == 3 and np.array_equal(ref.table(3, 5), _literal(T_3_5, 3))
    assert ref.ksize(720, 540) == 5 and int(ref.table(720, 540)[:, 1].max()) == 3  # at most three live taps
    ident = ref.table(540, 540)
    # the identity: one tap of 2^22 on the pixel itself (the row may list a second, zero-weight tap)
    assert np.array_equal(ident[:, 0], np.arange(540)) and (ident[:, 2] == 1 << 22).all() and not ident[:, 3:].any()


def test_restatement_equals_the_golden_file(golden):
    assert [tuple(int(v) for v in s) for s in golden["sizes"]] == [(*a, *b) for a, b in ref.GOLDEN_CASES]
    for i, ((hin, win), size) in enumerate(ref.GOLDEN_CASES):
        for kind, binary in (("rand", False), ("bin", True)):
            img = golden[f"in_{kind}_{i}"]
            assert np.array_equal(img, ref.make_image(i, hin, win, binary)), "the generator moved away from the file"
            got, want = ref.resize(img, size), golden[f"out_{kind}_{i}"]
            assert got.shape == want.shape == size and got.dtype == np.uint8
            assert np.array_equal(got, want), (i, kind, int(np.abs(got.astype(int) - want).max()))
    assert np.array_equal(golden["stripes_in"], ref.STRIPES) and np.array_equal(golden["stripes_out"], ref.STRIPES_OUT)
    assert np.array_equal(ref.resize(ref.STRIPES, (1, 6)), ref.STRIPES_OUT)


def test_restatement_equals_pillow_live():
    pil = pytest.importorskip("PIL.Image")

    def pillow(img, size):
        return np.array(pil.fromarray(img).resize((size[1], size[0]), resample=pil.BILINEAR))

    for i, ((hin, win), size) in enumerate(ref.GOLDEN_CASES):
        for binary in (False, True):
            img = ref.make_image(i, hin, win, binary)
            assert np.array_equal(ref.resize(img, size), pillow(img, size)), (i, binary)
    assert np.array_equal(pillow(ref.STRIPES, (1, 6)), ref.STRIPES_OUT)
    img = ref.make_image(99, 720, 1280)
    assert np.array_equal(ref.resize(img, (540, 960)), pillow(img, (540, 960)))


def test_restatement_handles_batches_and_the_float_image():
    imgs = np.stack([ref.make_image(s, 20, 31) for s in range(3)])
    both = ref.resize(imgs, (15, 23))
    for k in range(3):
        assert np.array_equal(both[k], ref.resize(imgs[k], (15, 23)))
    levels = np.arange(256, dtype=np.uint8)
    # the plain fp32 division gives the bits of float32(float64(v) / 255) for every level
    assert np.array_equal(ref.unit(levels).view(np.uint32), (levels.astype(np.float32) / np.float32(255)).view(np.uint32))
    assert np.array_equal(torch.from_numpy(ref.unit(levels)), torch.from_numpy(levels).float() / 255)


# ---- the library's tables --------------------------------------------------------------------------------------------------
def _lib_table(handle, in_size, out_size):
    ks = handle.az_resample_bilinear_ksize(in_size, out_size)
    assert ks > 0, (in_size, out_size, ks)
    buf = np.full(out_size * (2 + ks) + 1, 0x5A5A5A5A, np.int32)
    assert handle.az_resample_bilinear_table(buf.ctypes.data, in_size, out_size) == 0
    assert buf[-1] == 0x5A5A5A5A
    return ks, buf[:-1].reshape(out_size, 2 + ks)


def test_new_symbols_are_exported_and_typed(handle):
    declared = _lib.declared_symbols()
    for name in NEW:
        assert name in declared, f"{name} missing from include/azhip.h"
        assert getattr(handle, name).argtypes == _lib._SIGS[name]
        assert getattr(handle, name).restype is ctypes.c_int
    assert _lib.expected_abi_version() == 6 and handle.az_abi_version() == 6  # additive change


@pytest.mark.parametrize("in_size,out_size", PAIRS)
def test_library_tables_equal_the_restatement(handle, in_size, out_size):
    ks, tab = _lib_table(handle, in_size, out_size)
    assert ks == ref.ksize(in_size, out_size)
    assert np.array_equal(tab, ref.table(in_size, out_size))


def test_library_tables_equal_the_literal_values_and_refuse_what_they_document(handle):
    assert np.array_equal(_lib_table(handle, 8, 6)[1], _literal(T_8_6, 5))
    assert np.array_equal(_lib_table(handle, 3, 5)[1], _literal(T_3_5, 3))
    assert _lib_table(handle, 64, 8)[0] == 17 and _lib_table(handle, 200, 25)[0] == 17  # at the cap
    word = np.full(1, 7, np.int32)
    assert handle.az_resample_bilinear_ksize(65, 8) == EUNSUP
    assert handle.az_resample_bilinear_table(word.ctypes.data, 65, 8) == EUNSUP
    for i, o in ((0, 8), (8, 0), (-1, 8), (8, -5), (0, 0)):
        assert handle.az_resample_bilinear_ksize(i, o) == EINVAL
        assert handle.az_resample_bilinear_table(word.ctypes.data, i, o) == EINVAL
    assert handle.az_resample_bilinear_table(None, 8, 6) == EINVAL
    assert word[0] == 7


def test_argument_validation_happens_before_any_launch(handle):
    buf = (ctypes.c_float * 16)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    # az_resize_bilinear_u8(out_u8, out_f32, img, table_y, table_x, N, Hin, Win, Hout, Wout, y0, x0, h, w, stream)
    rs = handle.az_resize_bilinear_u8
    assert rs(p, p, None, p, p, 1, 97, 131, 73, 98, 0, 0, 73, 98, None) == EINVAL
    assert rs(p, p, p, None, p, 1, 97, 131, 73, 98, 0, 0, 73, 98, None) == EINVAL
    assert rs(p, p, p, p, None, 1, 97, 131, 73, 98, 0, 0, 73, 98, None) == EINVAL
    assert rs(None, None, p, p, p, 1, 97, 131, 73, 98, 0, 0, 73, 98, None) == EINVAL
    for n in (0, -1):
        assert rs(p, None, p, p, p, n, 97, 131, 73, 98, 0, 0, 73, 98, None) == EINVAL
    for dims in ((0, 131, 73, 98), (97, 0, 73, 98), (97, 131, 0, 98), (97, 131, 73, -2)):
        assert rs(p, None, p, p, p, 1, *dims, 0, 0, 1, 1, None) == EINVAL
    for win in ((-1, 0, 5, 5), (0, -1, 5, 5), (0, 0, 0, 5), (0, 0, 5, 0), (0, 0, 74, 98), (0, 0, 73, 99), (72, 97, 2, 1),
                (72, 97, 1, 2), (73, 0, 1, 1), (0, 98, 1, 1), (1, 0, 2 ** 31 - 1, 1)):
        assert rs(None, p, p, p, p, 1, 97, 131, 73, 98, *win, None) == EINVAL, win
    assert rs(p, None, p, p, p, 1, 65, 131, 8, 98, 0, 0, 8, 98, None) == EUNSUP   # rows: 65 > 8 * 8
    assert rs(p, None, p, p, p, 1, 97, 200, 73, 24, 0, 0, 73, 24, None) == EUNSUP  # columns: 200 > 8 * 24


def test_python_surface_refuses_what_it_cannot_run(handle):
    from activezero_amd.datasets import dataset_utils_gpu as du

    u8 = torch.zeros(24, 29, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        du.resize_bilinear(u8, (18, 22))
    with pytest.raises(RuntimeError, match="GPU"):
        du.resize_bilinear(torch.zeros(2, 24, 29, dtype=torch.uint8), (18, 22), crop=(1, 2, 3, 4), dtype=torch.float32)
    with pytest.raises(RuntimeError, match="expected torch.uint8"):
        du.resize_bilinear(torch.zeros(24, 29), (18, 22))
    with pytest.raises(RuntimeError, match=r"\[Hin,Win\] or \[B,Hin,Win\]"):
        du.resize_bilinear(torch.zeros(1, 2, 24, 29, dtype=torch.uint8), (18, 22))
    with pytest.raises(RuntimeError, match=r"\[Hin,Win\] or \[B,Hin,Win\]"):
        du.resize_bilinear(torch.zeros(29, dtype=torch.uint8), (18, 22))
    for crop in ((0, 0, 19, 22), (0, 0, 18, 23), (17, 21, 2, 1), (-1, 0, 4, 4), (0, 0, 0, 4)):
        with pytest.raises(RuntimeError, match="outside"):
            du.resize_bilinear(u8, (18, 22), crop=crop)
    with pytest.raises(RuntimeError, match="ratio above 8"):
        du.resize_bilinear(u8, (2, 22))  # 24 > 8 * 2
    with pytest.raises(RuntimeError, match="ratio above 8"):
        du.resize_bilinear(torch.zeros(24, 65, dtype=torch.uint8), (18, 8))
    with pytest.raises(RuntimeError, match="positive"):
        du.resize_bilinear(u8, (0, 22))
    with pytest.raises(RuntimeError, match="dtype"):
        du.resize_bilinear(u8, (18, 22), dtype=torch.float64)
    with pytest.raises(TypeError):
        du.resize_bilinear(np.zeros((24, 29), np.uint8), (18, 22))
    assert du._RESAMPLE_TABLES == {}  # nothing was built or copied on the way to a refusal
    # the dataset takes the keyword without touching a device, and refuses sizes that 0.75 does not map onto the item's
    from activezero_amd.datasets.messytable_synthetic import SyntheticMessytableDataset
    assert SyntheticMessytableDataset(length=1, device="cpu").real_size is None
    assert SyntheticMessytableDataset(length=1, device="cpu", height=36, width=48, real_size=(48, 64)).real_size == (48, 64)
    assert SyntheticMessytableDataset(length=1, device="cpu", height=540, width=960, real_size=(720, 1280)).real_size == (720, 1280)
    with pytest.raises(RuntimeError, match="0.75"):
        SyntheticMessytableDataset(length=1, device="cpu", height=36, width=48, real_size=(48, 66))
    with pytest.raises(RuntimeError, match="0.75"):
        SyntheticMessytableDataset(length=1, device="cpu", real_size=(256, 512))
