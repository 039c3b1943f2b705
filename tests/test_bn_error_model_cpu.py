"""CPU: the checks of tests/_bn_fp64ref.py are sharp enough to catch a subtly wrong BatchNorm kernel.

The fp32 emulations of that module (the documented tile, block and merge structure of csrc/az_bn3d.hip, in torch) pass every
check at small cases of every channel count; each mutant -- one defect of a class a kernel could have -- fails at least one.
The worst ratios of the emulations are printed: twice those of the random-walk checks are the (b) constants of the module.
No kernel is built or run."""
import pytest
import torch

from tests import _bn_fp64ref as R

EPS, MOM = 1e-5, 0.1
# (C, nvox, groups): fewer voxels than a block, ragged blocks, several statistics tiles, the reduce-block cap from both sides
CASES = [(32, 7, 1), (64, 7, 3), (128, 1003, 1), (32, 1003, 2), (64, 5000, 2), (32, 512 * 32 - 1, 2), (128, 128 * 8 + 8 + 3, 3),
         (64, 256 * 16 + 16 + 3, 1)]


def chain(C, V, G, seed=900, stats_mut=None, fin_mut=None, apply_mut=None, bwd_mut=None, saved_y=False, grid=None):
    """the whole emulated layer on one input set -> dict of every check's ratio"""
    x, dy, res, gamma, beta = R.make_inputs(G, V, C, seed + C + V + G)
    out = {}
    part, cnt = R.emu_stats(x, stats_mut)
    out.update(R.check_stats(part, cnt, x))
    part, cnt = R.emu_stats(x)
    rm, rv = torch.linspace(-1.0, 1.0, C), torch.linspace(0.5, 2.0, C)
    fin = R.emu_finalize(part, cnt, gamma, beta, rm, rv, EPS, MOM, mutant=fin_mut)
    out.update(R.check_finalize(fin, part, cnt, gamma, beta, rm, rv, EPS, MOM))
    fin = R.emu_finalize(part, cnt, gamma, beta, rm, rv, EPS, MOM)
    sc, sh = fin["scale"], fin["shift"]
    r = res if saved_y else None
    y = R.emu_apply(x, sc, sh, r, True, grid=grid, mutant=apply_mut)
    out.update(R.check_apply(y, x, sc, sh, r, True))
    y = R.emu_apply(x, sc, sh, r, True)
    for relu in (False, True):
        a = (None, None) if (saved_y or not relu) else (sc, sh)
        got = R.emu_bwd(dy, x, y if saved_y else None, fin["mean"], fin["invstd"], gamma, a[0], a[1], relu, mutant=bwd_mut)
        mask = R.relu_mask(x, a[0], a[1], y) if relu else None
        ck = R.check_bwd(got, dy, x, fin["mean"], fin["invstd"], gamma, mask)
        out.update({k + ("_relu" if relu else ""): v for k, v in ck.items()})
    return out


def test_the_emulations_pass_every_check(capsys):
    worst = {}
    for C, V, G in CASES:
        for saved_y in (False, True):
            for k, v in chain(C, V, G, saved_y=saved_y).items():
                k = k.replace("_relu", "")
                if v > worst.get(k, (0.0,))[0]:
                    worst[k] = (v, (C, V, G, saved_y))
    with capsys.disabled():
        print()
        for k in sorted(worst):
            scale = {"stats_mean_b": R.CB_STATS_MEAN, "stats_m2_b": R.CB_STATS_M2, "dbeta_b": R.CB_BWD_SUM, "dgamma_b": R.CB_BWD_SUM}.get(k)
            note = f"  (x {scale} = {worst[k][0] * scale:.3f} of the un-scaled random walk)" if scale else ""
            print(f"emulation worst {k:14s} {worst[k][0]:.3f} at (C, nvox, groups, saved y) = {worst[k][1]}{note}")
    for k, (v, case) in worst.items():
        assert v <= 1.0, (k, v, case)
    # the (b) constants are twice the emulations' worst: the worst ratio against them is one half (to the printed digits)
    for k in ("stats_mean_b", "stats_m2_b", "dbeta_b", "dgamma_b"):
        assert worst[k][0] <= 0.5 + 1e-2, (k, worst[k])
    assert max(worst["stats_mean_b"][0], 0) >= 0.5 - 1e-2 and worst["stats_m2_b"][0] >= 0.5 - 1e-2
    assert max(worst["dbeta_b"][0], worst["dgamma_b"][0]) >= 0.5 - 1e-2


def test_the_two_stage_finalize_emulation_passes_and_agrees_with_the_single_stage():
    torch.manual_seed(5)
    C, T = 32, 4100
    cnt = torch.randint(0, 30, (1, T)).float()
    cnt[0, 3 * 129:4 * 129] = 0.0   # one whole slice of empty tiles
    tm = 1e3 + torch.randn(1, C, T)
    part = torch.stack([tm * cnt[:, None, :], torch.rand(1, C, T) * cnt[:, None, :]], -1)
    gamma, beta = torch.rand(C) + 0.5, torch.rand(C) - 0.5
    rm, rv = torch.zeros(C), torch.ones(C)
    for two in (False, True):
        fin = R.emu_finalize(part, cnt, gamma, beta, rm, rv, EPS, MOM, two_stage=two)
        ck = R.check_finalize(fin, part, cnt, gamma, beta, rm, rv, EPS, MOM, two_stage=two)
        assert R.worst(ck) <= 1.0, (two, ck)
    bad = R.emu_finalize(part, cnt, gamma, beta, rm, rv, EPS, MOM, two_stage=True, mutant="slice_dropped")
    assert R.worst(R.check_finalize(bad, part, cnt, gamma, beta, rm, rv, EPS, MOM, two_stage=True)) > 1.0


MUTANTS = [
    ("one statistics tile dropped", dict(stats_mut="tile_dropped"), (64, 5000, 2)),
    ("a ragged tile counted as full", dict(stats_mut="ragged_full"), (128, 1003, 1)),
    ("M2 merged without the n (mean_t - mean)^2 term", dict(fin_mut="no_delta_term"), (64, 5000, 2)),
    ("biased variance written to running_var", dict(fin_mut="biased_var"), (32, 1003, 2)),
    ("group g reading group 0's partials", dict(fin_mut="group0_partials"), (32, 1003, 2)),
    ("running statistics updated in reverse group order", dict(fin_mut="reverse_groups"), (32, 1003, 2)),
    ("mul then add in place of fma in apply", dict(apply_mut="mul_add"), (32, 1003, 2)),
    ("the ReLU mask taken with >=", dict(bwd_mut="mask_ge", saved_y=True), (32, 1003, 2)),
    ("the mean(dz) term dropped from dx", dict(bwd_mut="no_mean_dz"), (32, 1003, 2)),
    ("k2 taken from the other group", dict(bwd_mut="k2_other_group"), (32, 1003, 2)),
    ("dgamma not summed over the groups", dict(bwd_mut="dgamma_group0"), (32, 1003, 2)),
    ("the last stride voxels reduced twice", dict(bwd_mut="tail_twice"), (32, 512 * 32 - 1 + 40, 2)),
    ("one grid-stride trip of apply skipped", dict(apply_mut="trip_skipped", grid=3), (32, 1003, 2)),
]


@pytest.mark.parametrize("name,kw,case", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_each_mutant_fails_a_check(name, kw, case):
    C, V, G = case
    clean = chain(C, V, G, saved_y=kw.get("saved_y", False))
    assert max(clean.values()) <= 1.0, clean
    bad = chain(C, V, G, **kw)
    failed = [k for k, v in bad.items() if v > 1.0]
    assert failed, (name, bad)
