"""CPU: the helpers of tests/_nonfinite.py see the defects tests/test_gpu_nonfinite.py is there for, and torch -- the reference
of those tests -- treats non-finite values the way include/azhip.h ("Non-finite values") says the reference does."""
import pytest
import torch
import torch.nn.functional as F

from tests import _nonfinite as NF

NAN, INF = float("nan"), float("inf")


def test_classes_and_counts():
    t = torch.tensor([[0.0, NAN, INF], [-INF, -0.0, 3.0e38]])
    assert NF.classes(t).tolist() == [[0, 1, 2], [3, 0, 0]] and NF.classes(t).dtype == torch.int8
    assert NF.counts(NF.classes(t)) == [3, 1, 1, 1]
    assert NF.finite_amax(t) == pytest.approx(3.0e38) and NF.finite_amax(torch.tensor([NAN, INF])) == 0.0


def test_the_reference_keeps_nan_and_maps_inf_point_wise():
    x = torch.tensor([NAN, INF, -INF], dtype=torch.float64)
    assert NF.classes(F.relu(x)).tolist() == [NF.NAN, NF.PINF, NF.FINITE] and float(F.relu(x)[2]) == 0.0
    assert NF.classes(torch.clip(x, 0, 100)).tolist() == [NF.NAN, NF.FINITE, NF.FINITE] and float(torch.clip(x, 0, 100)[1]) == 100.0
    v = torch.randn(2, 3, 4, 5, 6, dtype=torch.float64)
    v[1, 2, 0, 1, 2] = NAN
    y = F.relu(torch.nn.BatchNorm3d(3).double().train()(v))
    assert bool(torch.isnan(y[:, 2]).all()) and not bool(torch.isnan(y[:, :2]).any())
    p = torch.tensor([0.25, NAN, 7.0], dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(F.smooth_l1_loss(p, torch.zeros(3, dtype=torch.float64)), p)
    assert NF.classes(g).tolist() == [NF.FINITE, NF.NAN, NF.FINITE]


def test_same_classes_sees_a_swallowed_nan_and_a_nan_turned_inf(capsys):
    ref = torch.tensor([1.0, NAN, 0.0, INF], dtype=torch.float64)
    NF.same_classes(torch.tensor([1.5, NAN, 0.0, INF]), ref, "equal classes, other values")
    assert "got [finite 2 nan 1 +inf 1 -inf 0]" in capsys.readouterr().out
    for wrong in ([1.0, 0.0, 0.0, INF],      # relu written fmaxf(y, 0): the NaN became 0
                  [1.0, -INF, 0.0, INF],     # a floor of -inf
                  [1.0, NAN, 0.0, 3.4e38],   # an inf clamped to a finite bound
                  [NAN, NAN, 0.0, INF]):     # a NaN where the reference has none
        with pytest.raises(AssertionError, match="differ in class"):
            NF.same_classes(torch.tensor(wrong), ref, "defect")
    with pytest.raises(AssertionError):
        NF.same_classes(torch.zeros(3), ref, "shape")


def test_untouched_is_equality_of_bits():
    clean = torch.tensor([1.0, 2.0, 0.0, 4.0])
    keep = torch.tensor([True, True, True, False])
    NF.untouched(torch.tensor([1.0, 2.0, 0.0, NAN]), clean, keep, "ok")
    with pytest.raises(AssertionError, match="1 of 3"):
        NF.untouched(torch.tensor([1.0, 2.0000002, 0.0, NAN]), clean, keep, "one ulp")
    with pytest.raises(AssertionError, match="1 of 3"):
        NF.untouched(torch.tensor([1.0, 2.0, -0.0, NAN]), clean, keep, "the sign of zero")
    with pytest.raises(AssertionError, match="nothing is left"):
        NF.untouched(clean, clean, torch.zeros(4, dtype=torch.bool), "empty")


def test_all_nan():
    where = torch.tensor([[True, False]])
    NF.all_nan(torch.tensor([[NAN, 1.0], [NAN, 2.0]]), where, "ok")
    with pytest.raises(AssertionError, match="1 of 2"):
        NF.all_nan(torch.tensor([[NAN, 1.0], [-INF, 2.0]]), where, "a NaN turned -inf")


def test_reads_follows_the_layers_index_map():
    m = torch.zeros(1, 1, 4, 6, 8, dtype=torch.bool)
    m[0, 0, 2, 3, 4] = m[0, 0, 0, 0, 0] = True
    r = NF.reads(m, lambda x, w: F.conv3d(x, w, padding=1))
    assert r.shape == m.shape and int(r.sum()) == 27 + 8 and bool(r[0, 0, 1:4, 2:5, 3:6].all()) and bool(r[0, 0, :2, :2, :2].all())
    r = NF.reads(m, lambda x, w: F.conv3d(x, w, stride=2, padding=1))  # output o reads 2 o - 1 .. 2 o + 1
    assert tuple(r.shape) == (1, 1, 2, 3, 4) and r.nonzero()[:, 2:].tolist() == [[0, 0, 0], [1, 1, 2], [1, 2, 2]]
    r = NF.reads(m, lambda x, w: F.conv_transpose3d(x, w, stride=2, padding=1, output_padding=1))  # input i reaches 2 i - 1 .. 2 i + 1
    assert tuple(r.shape) == (1, 1, 8, 12, 16) and int(r.sum()) == 27 + 8 and bool(r[0, 0, 3:6, 5:8, 7:10].all())
    m2 = torch.zeros(1, 1, 5, 7, dtype=torch.bool)
    m2[0, 0, 4, 6] = True
    assert int(NF.reads(m2, lambda x, w: F.conv2d(x, w, padding=1)).sum()) == 4
