"""The BatchNorm kernels of csrc/az_bn3d.hip against fp64 in every launch regime (references, bounds and the derivation of
every figure: tests/_bn_fp64ref.py; that the checks would see a wrong kernel: tests/test_bn_error_model_cpu.py).

Every branch of that file is chosen by tensor size.  The cases below are the smallest sizes that reach each regime, per channel
count (VPB = 256 / (C / 4) voxels per block): fewer voxels than one block, ragged last blocks, the backward reduce pass at and
past its block cap, the backward apply pass at its grid cap, a forward apply that walks its grid more than once, the statistics
tiles at their cap, the finalize step with 1 ... 9001 tiles on one and on two stages, and the nontemporal kernels at, below
and past their 256 MB threshold.  Inputs carry a channel whose mean is 10^3 standard deviations, a constant channel, a channel
the ReLU switches off entirely, and a gradient with 300x spikes.  The C ABI is called through activezero_amd.ops._call."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from activezero_amd import _lib, amax, bn2d  # noqa: E402
from activezero_amd.ops import _call, _p, _stream  # noqa: E402
from tests import _bn_fp64ref as R  # noqa: E402

DEV = torch.device("cuda:0")
EPS, MOM = 1e-5, 0.1
WORST = {}

ALL_REGIMES = {"one_tile_below_vpb", "ragged_block", "bwd_reduce_cap", "bwd_apply_cap", "apply_trips", "stats_tile_cap", "nontemporal",
               "finalize_1", "finalize_below_1024", "finalize_above_1024", "finalize_4095", "finalize_4096"}


def _cases():
    """(C, nvox per group, the regimes the case is there for)"""
    out = []
    for C, big1, big2 in ((32, 40013, 140003), (64, 20011, 70001), (128, 10007, 35003)):
        v, cap = R.vpb(C), R.bwd_cap(C)
        out += [(C, 7, {"one_tile_below_vpb", "ragged_block"}), (C, 1003, {"ragged_block"}),
                (C, cap * v - 1, {"bwd_reduce_cap", "ragged_block"}), (C, cap * v + v + 3, {"bwd_reduce_cap", "ragged_block"}),
                (C, big1, {"bwd_apply_cap", "bwd_reduce_cap"}), (C, big2, {"apply_trips", "bwd_apply_cap"})]
    out.append((128, 262149, {"stats_tile_cap", "apply_trips"}))
    return out


def _nt_cases():
    out = []
    for C in R.CHANNELS:
        t = R.NT_BYTES // (4 * C)
        out += [(C, t, {"nontemporal"}), (C, t - 1, {"ragged_block", "apply_trips"}), (C, t + 3, {"nontemporal", "ragged_block"})]
    return out


CASES, NT_CASES = _cases(), _nt_cases()
FINALIZE_TILES = (1, 37, 1500, 4095, 4096, 4097, 9001)


def _finalize_regimes(T):
    r = set()
    if T == 1:
        r.add("finalize_1")
    elif T < 1024:
        r.add("finalize_below_1024")
    elif T < 4095:
        r.add("finalize_above_1024")
    if T == 4095:
        r.add("finalize_4095")
    if T >= R.TWO_STAGE_TILES:
        r.add("finalize_4096")
    return r


@pytest.fixture(autouse=True)
def _free():
    yield
    torch.cuda.empty_cache()


def _record(tag, ratios, capsys=None):
    for k, v in ratios.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    if capsys is not None:
        with capsys.disabled():
            print(f"\n  {tag}: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(ratios.items())), end="")
    bad = {k: v for k, v in ratios.items() if k not in R.PASS_KEYS_EXCLUDED and not v <= 1.0}
    assert not bad, (tag, bad)


def _assert_regime(C, V, want):
    """the case is where it claims to be, by the library's own launch arithmetic"""
    lib = _lib.lib()
    got = R.regimes(V, C)
    assert want <= got, (C, V, want, got)
    assert lib.az_bn3d_stats_tiles(V, C) == R.stats_tiles(V, C)
    assert lib.az_bn3d_bwd_workspace(V, C) == 2 * R.bwd_blocks_uncapped(V, C) * C * 2 * 4
    for G in (1, 3):
        fwd = G * (C * R.stats_tiles(V, C) * 2 + R.stats_tiles(V, C))
        bwd = G * (R.bwd_blocks_uncapped(V, C) * C * 2 + C * 3)
        assert lib.az_bn2d_workspace(G, V, C) == 4 * max(fwd, bwd)
    t = R.NT_BYTES // (4 * C)
    assert R.nontemporal(V, C) == (V >= t)
    if "bwd_reduce_cap" in want:
        assert R.bwd_blocks(V, C) == R.bwd_cap(C) and (V + R.vpb(C) - 1) // R.vpb(C) >= R.bwd_cap(C)
    if "apply_trips" in want:
        assert V * C // 4 > R.GRID_CAP * 256
    if "bwd_apply_cap" in want:
        assert R.bwd_apply_grid(V, C) == R.BWD_APPLY_CAP and V * C // 4 > R.BWD_APPLY_CAP * 256
    if "stats_tile_cap" in want:
        assert R.stats_tiles(V, C) == R.STATS_TILE_CAP and -(-V // (R.STATS_TILE_CAP * R.vpb(C))) > 16


def test_the_cases_reach_every_regime():
    seen = set()
    for C, V, want in CASES + NT_CASES:
        assert want <= R.regimes(V, C), (C, V)
        seen |= want
    for T in FINALIZE_TILES:
        seen |= _finalize_regimes(T)
    assert seen == ALL_REGIMES, ALL_REGIMES - seen
    for C in R.CHANNELS:  # ... and each size-driven one for every channel count
        mine = set().union(*[w for c, _, w in CASES + NT_CASES if c == C])
        assert ALL_REGIMES - mine <= {"stats_tile_cap"} | {r for r in ALL_REGIMES if r.startswith("finalize")}, (C, mine)
        # (the nontemporal sizes are past the statistics tile cap for every C, by the arithmetic)
        assert "stats_tile_cap" in R.regimes(R.NT_BYTES // (4 * C), C)


# ---- the kernels through the C ABI --------------------------------------------------------------------------------------------
def k_stats(x):
    _, V, C = x.shape
    T = R.stats_tiles(V, C)
    part, cnt = torch.full((1, C, T, 2), float("nan"), device=DEV), torch.full((1, T), float("nan"), device=DEV)
    _call("az_bn3d_stats", _p(part), _p(cnt), _p(x), V, C, _stream())
    return part, cnt


def k_finalize(part, cnt, gamma, beta, rm, rv, nbt, scratch=False):
    _, C, T, _ = part.shape
    o = torch.full((4, 1, C), float("nan"), device=DEV)
    rm, rv = (rm.clone(), rv.clone()) if rm is not None else (None, None)
    sc = torch.empty(int(_lib.lib().az_bn3d_finalize_scratch(C)), device=DEV) if scratch else None
    _call("az_bn3d_finalize", _p(o[0]), _p(o[1]), _p(o[2]), _p(o[3]), _p(rm), _p(rv), _p(part), _p(cnt), _p(gamma), _p(beta), T, C, EPS,
          MOM, _p(nbt), _p(sc), sc.numel() if scratch else 0, _stream())
    got = {"mean": o[0], "invstd": o[1], "scale": o[2], "shift": o[3]}
    if rm is not None:
        got["running_mean"], got["running_var"] = rm, rv
    return got


def k_apply(x, scale, shift, res, relu):
    _, V, C = x.shape
    y = torch.full_like(x, float("nan"))
    am = torch.zeros(amax.AMAX_SLOTS, device=DEV)
    _call("az_bn3d_apply", _p(y), _p(x), _p(scale), _p(shift), _p(res), int(relu), V, C, _p(am), _stream())
    assert float(am[::64].max()) == float(y.abs().max())
    return y


def k_bwd3d(dy, x, y, mean, invstd, gamma, scale, shift, relu, want_dz, split):
    _, V, C = x.shape
    wsb = _lib.lib().az_bn3d_bwd_workspace(V, C)
    ws = torch.empty(wsb // 4, device=DEV)
    dx = torch.full_like(x, float("nan"))
    dz = torch.full_like(x, float("nan")) if want_dz else None
    dg, db, coef = (torch.full((n,), float("nan"), device=DEV) for n in (C, C, 3 * C))
    am = torch.full((amax.AMAX_SLOTS,), 7.0, device=DEV)  # (need not be zero: the reduce pass clears it)
    _call("az_bn3d_bwd", _p(dx), _p(dz), _p(dg), _p(db), _p(coef), _p(ws), wsb, _p(dy), _p(y), _p(x), _p(mean), _p(invstd), _p(gamma),
          _p(scale), _p(shift), int(relu), V, C, _p(am), int(split), _stream())
    got = {"dx": dx, "dz": dz, "dgamma": dg, "dbeta": db, "coef": coef.view(1, C, 3)}
    if split:
        got["dx"], got["split_bound"] = R.decode_split(dx, am)
    else:
        assert float(am[::64].max()) == float(dx.abs().max())
    return got


def k_fwd2d(x, res, gamma, beta, rm, rv, nbt, relu):
    G, V, C = x.shape
    wsb = _lib.lib().az_bn2d_workspace(G, V, C)
    ws = torch.full((wsb // 4,), float("nan"), device=DEV)
    y = torch.full_like(x, float("nan"))
    o = torch.full((4, G, C), float("nan"), device=DEV)
    am = torch.zeros(amax.AMAX_SLOTS, device=DEV)
    _call("az_bn2d_fwd", _p(y), _p(o[0]), _p(o[1]), _p(o[2]), _p(o[3]), _p(rm), _p(rv), _p(x), _p(res), _p(gamma), _p(beta), _p(ws), wsb,
          int(relu), G, V, C, EPS, MOM, _p(nbt), None, None, 0, _p(am), _stream())
    T = R.stats_tiles(V, C)
    part = ws[:G * C * T * 2].view(G, C, T, 2).clone()
    cnt = ws[G * C * T * 2:G * C * T * 2 + G * T].view(G, T).clone()
    assert float(am[::64].max()) == float(y.abs().max())
    return y, {"mean": o[0], "invstd": o[1], "scale": o[2], "shift": o[3], "running_mean": rm, "running_var": rv}, part, cnt


def k_bwd2d(dy, x, y, mean, invstd, gamma, scale, shift, relu, want_dz):
    G, V, C = x.shape
    wsb = _lib.lib().az_bn2d_workspace(G, V, C)
    ws = torch.full((wsb // 4,), float("nan"), device=DEV)
    dx = torch.full_like(x, float("nan"))
    dz = torch.full_like(x, float("nan")) if want_dz else None
    dg, db = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    am = torch.zeros(amax.AMAX_SLOTS, device=DEV)
    _call("az_bn2d_bwd", _p(dx), _p(dz), _p(dg), _p(db), _p(ws), wsb, _p(dy), _p(y), _p(x), _p(mean), _p(invstd), _p(gamma), _p(scale),
          _p(shift), int(relu), G, V, C, _p(am), _stream())
    o = G * R.bwd_blocks_uncapped(V, C) * C * 2  # (the coefficients sit behind the uncapped partial area)
    assert float(am[::64].max()) == float(dx.abs().max())
    return {"dx": dx, "dz": dz, "dgamma": dg, "dbeta": db, "coef": ws[o:o + G * C * 3].view(G, C, 3).clone()}


def _layer(G, V, C, seed, two_d, capsys, tag):
    """statistics -> finalize -> apply (with and without residual) -> every backward variant, each step checked against the
    fp64 value of ITS inputs (the kernel outputs of the step before)"""
    x, dy, res, gamma, beta = R.make_inputs(G, V, C, seed, device=DEV)
    rm0, rv0 = torch.linspace(-1.0, 1.0, C, device=DEV), torch.linspace(0.5, 2.0, C, device=DEV)
    nbt = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    if two_d:
        rm, rv = rm0.clone(), rv0.clone()
        y_res, fin, part, cnt = k_fwd2d(x, res, gamma, beta, rm, rv, nbt, True)
        y = k_fwd2d(x, None, gamma, beta, None, None, None, True)[0]
        assert int(nbt) == 5 + G
    else:
        part, cnt = k_stats(x)
        fin = k_finalize(part, cnt, gamma, beta, rm0, rv0, nbt)
        assert int(nbt) == 6
        y, y_res = k_apply(x, fin["scale"], fin["shift"], None, True), k_apply(x, fin["scale"], fin["shift"], res, True)
    _record(tag + " stats", R.check_stats(part, cnt, x), capsys)
    _record(tag + " finalize", R.check_finalize(fin, part, cnt, gamma, beta, rm0, rv0, EPS, MOM), capsys)
    sc, sh, mean, invstd = fin["scale"], fin["shift"], fin["mean"], fin["invstd"]
    _record(tag + " apply", R.check_apply(y, x, sc, sh, None, True), capsys)
    _record(tag + " apply+res", R.check_apply(y_res, x, sc, sh, res, True), capsys)
    del y, res
    bwd = k_bwd2d if two_d else (lambda *a: k_bwd3d(*a, False))
    ref_plain = R.bwd_ref(dy, x, mean, invstd, gamma, None)
    plain = bwd(dy, x, None, mean, invstd, gamma, None, None, False, False)
    _record(tag + " bwd", R.check_bwd(plain, dy, x, mean, invstd, gamma, None, ref_plain), capsys)
    if not two_d:  # the same with dx written pre-split: against fp64, and the decode contract alone against the fp32 dx
        sp = k_bwd3d(dy, x, None, mean, invstd, gamma, None, None, False, False, True)
        ck = R.check_bwd(sp, dy, x, mean, invstd, gamma, None, ref_plain)
        ck.update(R.check_split_vs_fp32(sp["dx"], sp["split_bound"], plain["dx"]))
        assert torch.equal(sp["dgamma"], plain["dgamma"]) and torch.equal(sp["dbeta"], plain["dbeta"])
        _record(tag + " bwd split", ck, capsys)
        del sp
    del plain
    del ref_plain
    mask = R.relu_mask(x, sc, sh, None)
    ref = R.bwd_ref(dy, x, mean, invstd, gamma, mask)
    plain = bwd(dy, x, None, mean, invstd, gamma, sc, sh, True, True)
    _record(tag + " bwd remask", R.check_bwd(plain, dy, x, mean, invstd, gamma, mask, ref), capsys)
    if not two_d:
        sp = k_bwd3d(dy, x, None, mean, invstd, gamma, sc, sh, True, False, True)
        ck = R.check_bwd(sp, dy, x, mean, invstd, gamma, mask, ref)
        ck.update(R.check_split_vs_fp32(sp["dx"], sp["split_bound"], plain["dx"]))
        _record(tag + " bwd remask split", ck, capsys)
        del sp
    del plain
    del ref
    mask = R.relu_mask(x, None, None, y_res)
    assert bool((y_res == 0).any())  # (elements with y == 0 exactly are in: their gradient is 0)
    _record(tag + " bwd saved y", R.check_bwd(bwd(dy, x, y_res, mean, invstd, gamma, None, None, True, True), dy, x, mean, invstd, gamma, mask),
            capsys)


@pytest.mark.parametrize("C,V,want", CASES + NT_CASES, ids=[f"C{c}-{v}" for c, v, _ in CASES + NT_CASES])
def test_3d_entry_points(C, V, want, capsys):
    _assert_regime(C, V, want)
    _layer(1, V, C, 100 + C, False, capsys, f"3d C={C} nvox={V}")


@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("C,V,want", CASES, ids=[f"C{c}-{v}" for c, v, _ in CASES])
def test_2d_entry_points(C, V, want, G, capsys):
    _assert_regime(C, V, want)
    _layer(G, V, C, 200 + C + G, True, capsys, f"2d C={C} nvox={V} groups={G}")


@pytest.mark.parametrize("C", R.CHANNELS)
def test_nontemporal_apply_is_the_plain_apply_bit_for_bit(C):
    """threshold and threshold - 1 voxel: the two kernels differ in cache policy only"""
    t = R.NT_BYTES // (4 * C)
    assert R.nontemporal(t, C) and not R.nontemporal(t - 1, C)
    x, _, res, gamma, beta = R.make_inputs(1, t, C, 300 + C, device=DEV)
    sc, sh = gamma.view(1, C).contiguous(), beta.view(1, C).contiguous()
    for r in (None, res):
        y_nt = k_apply(x, sc, sh, r, True)
        y_pl = k_apply(x[:, :t - 1].contiguous(), sc, sh, None if r is None else r[:, :t - 1].contiguous(), True)
        assert torch.equal(y_nt[:, :t - 1].view(torch.int32), y_pl.view(torch.int32))
        del y_nt, y_pl


# ---- finalize on synthetic partials -------------------------------------------------------------------------------------------
def _synthetic_partials(T, C, seed, single=False):
    """partials of an fp64 tensor cut into T tiles of unequal counts (zero-count tiles, and one whole premerge slice of them)"""
    g = torch.Generator().manual_seed(seed)
    cnt = torch.randint(0, 25, (T,), generator=g)
    if T == 1:
        cnt[:] = 1 if single else 13
    elif single:
        cnt[:] = 0
        cnt[T // 3] = 1
    if T >= R.TWO_STAGE_TILES and not single:
        per = -(-T // R.PRE_SLICES)
        cnt[2 * per:3 * per] = 0
    N = int(cnt.sum())
    x = torch.randn(N, C, generator=g, dtype=torch.float64) * torch.linspace(0.01, 3.0, C, dtype=torch.float64)
    x += torch.linspace(-1e3, 1e3, C, dtype=torch.float64)
    x[:, 1] = 0.625  # a constant channel
    tile = torch.repeat_interleave(torch.arange(T), cnt)
    S = torch.zeros(T, C, dtype=torch.float64).index_add_(0, tile, x)
    mt = S / cnt.clamp_min(1)[:, None]
    M2 = torch.zeros(T, C, dtype=torch.float64).index_add_(0, tile, (x - mt[tile]) ** 2)
    part = torch.stack([S, M2], -1).permute(1, 0, 2).float().contiguous()
    return part[None].to(DEV), cnt.float()[None].to(DEV)


@pytest.mark.parametrize("single", [False, True], ids=["N", "N=1"])
@pytest.mark.parametrize("T", FINALIZE_TILES)
def test_finalize_on_synthetic_partials(T, single, capsys):
    C = 128 if T == 4096 else 32
    part, cnt = _synthetic_partials(T, C, 400 + T, single)
    gen = torch.Generator().manual_seed(T)
    gamma, beta = (torch.rand(C, generator=gen) + 0.5).to(DEV), (torch.rand(C, generator=gen) - 0.5).to(DEV)
    rm0, rv0 = torch.linspace(-2.0, 2.0, C, device=DEV), torch.linspace(0.5, 2.0, C, device=DEV)
    for scratch in (False, True):
        two = scratch and T >= R.TWO_STAGE_TILES
        for track in (True, False):
            nbt = torch.full((1,), 41, dtype=torch.int64, device=DEV)
            got = k_finalize(part, cnt, gamma, beta, rm0 if track else None, rv0 if track else None, nbt if track else None, scratch)
            _record(f"finalize T={T} C={C} N=1:{single} scratch={scratch} running={track}",
                    R.check_finalize(got, part, cnt, gamma, beta, rm0 if track else None, rv0 if track else None, EPS, MOM, two), capsys)
            assert int(nbt) == (42 if track else 41)


def test_finalize_rejects_a_scratch_one_float_short():
    lib = _lib.lib()
    C, T = 32, 4096
    part, cnt = _synthetic_partials(T, C, 1)
    o = torch.zeros(4, C, device=DEV)
    gamma = torch.ones(C, device=DEV)
    need = int(lib.az_bn3d_finalize_scratch(C))
    sc = torch.empty(need, device=DEV)
    code = lib.az_bn3d_finalize(_p(o[0]), _p(o[1]), _p(o[2]), _p(o[3]), None, None, _p(part), _p(cnt), _p(gamma), _p(gamma), T, C, EPS, MOM,
                                None, _p(sc), need - 1, _stream())
    assert lib.az_strerror(code) == b"AZ_EWORKSPACE"


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("has_res", [False, True])
def test_bn_act_is_the_c_abi_bit_for_bit(has_res):
    """bn2d.bn_act (its workspace sizing, its choice of the mask path) against the direct calls checked above; two groups of
    2 x 47 x 45 = 4230 voxels of 64 channels: past the backward reduce cap (256 blocks of 16)"""
    G, n, C, h, w = 2, 4, 64, 47, 45
    V = (n // G) * h * w
    assert "bwd_reduce_cap" in R.regimes(V, C)
    xr, dyr, resr, gamma, beta = R.make_inputs(G, V, C, 500, device=DEV)
    nchw = lambda t: t.view(n, h, w, C).permute(0, 3, 1, 2)  # noqa: E731  (channels_last memory)
    bn = torch.nn.BatchNorm2d(C).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    x = nchw(xr).detach().requires_grad_()
    res = nchw(resr).detach().requires_grad_() if has_res else None
    y = bn2d.bn_act(x, bn, relu=True, residual=res, groups=G)
    y.backward(nchw(dyr))
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
    y2, fin, _, _ = k_fwd2d(xr, resr if has_res else None, gamma, beta, rm, rv, nbt, True)
    a = (None, None) if has_res else (fin["scale"], fin["shift"])
    got = k_bwd2d(dyr, xr, y2 if has_res else None, fin["mean"], fin["invstd"], gamma, a[0], a[1], True, has_res)
    bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731
    assert torch.equal(bits(y.permute(0, 2, 3, 1)), bits(y2.view(n, h, w, C)))
    assert torch.equal(bits(x.grad.permute(0, 2, 3, 1)), bits(got["dx"].view(n, h, w, C)))
    assert torch.equal(bits(bn.weight.grad), bits(got["dgamma"])) and torch.equal(bits(bn.bias.grad), bits(got["dbeta"]))
    assert torch.equal(bits(bn.running_mean), bits(rm)) and torch.equal(bits(bn.running_var), bits(rv))
    assert int(bn.num_batches_tracked) == int(nbt) == G
    if has_res:
        assert torch.equal(bits(res.grad.permute(0, 2, 3, 1)), bits(got["dz"].view(n, h, w, C)))


def test_zz_print_the_worst_ratios(capsys):
    """(runs last in this file: the record copied into tests/_bn_fp64ref.py's GPU_RECORD)"""
    with capsys.disabled():
        print("\nworst ratios: " + ", ".join(f'"{k}": {v:.3f}' for k, v in sorted(WORST.items())))
