"""fp64 references, error bounds and fp32 emulations of the BatchNorm kernels of csrc/az_bn3d.hip (shared by
tests/test_bn_error_model_cpu.py and tests/test_gpu_bn_fp64.py; a helper module, not a conftest).

Tensors are channels-last with a leading statistic-group axis: x, dy, y, residual [G, nvox, C]; per-channel vectors [G, C];
statistics partials [G, C, T, 2] = (sum, centred M2) with counts [G, T] (the layout az_bn3d_finalize consumes).  Every
reference is the fp64 value of the operation on the SAME fp32 inputs the kernel got, in plain torch elementwise operations
and reductions (CPU or GPU).  Every check is a ratio error / bound per element or per channel, of which the largest is
returned: 1 or less passes, a bound of 0 demands an error of 0, a non-finite output is ratio inf.  u = 2^-24.

apply (az_bn3d_apply, the apply pass of az_bn2d_fwd):   y = max(fl(fl(fma(x, sc, sh)) + r), 0)
    t = x sc + sh in fp64.  Two roundings, no constant: |y - ref| <= (u |t| + u |t + r|) (1 + 2^-20); without a residual the
    second rounding does not happen and the bound is u |t| (1 + 2^-20).  A kernel that rounds the product x sc before it adds
    sh is off by up to u |x sc|, which this bound refuses wherever x sc and sh cancel.

finalize (az_bn3d_finalize, the finalize pass of az_bn2d_fwd), against the fp64 Chan merge of the fp32 partials.  The kernel
    merges in fp64, so what is left are the fp32 roundings of its outputs:
      mean          1   (float)mu
      invstd        1   (float)istd
      scale         2   gamma * fl(istd)
      shift         5   fl(mu), fl(mu) * scale (scale carries its 2), the subtraction from beta: 4 u |mu scale| + u |shift|
      running_mean  5   fl(1 - m), its product with the old value, fl(mu), its product with m, the sum:
                        2 u |(1 - m) old| + 2 u |m mu| + u |new|; the bound of the old value is carried over times (1 - m)
                        when the groups update it one after the other
      running_var   5   the same with the unbiased M2 / (N - 1) (N = 1: M2 / N)
    Two-stage path (ntiles >= 4096 with scratch): the 32 slice partials (S_s, M2_s about the slice mean) are rounded to fp32
    in between, which adds  u sum_s |S_s| / N  to the mean and  u sum_s (M2_s + 2 |mean_s - mean| |S_s|)  to M2 (the second
    term: a slice sum that moves shifts the slice mean in the n_s (mean_s - mean)^2 term of the merge); both are propagated
    through invstd = (M2 / N + eps)^-1/2, scale and shift.  num_batches_tracked rises by `groups`, exactly.

statistics producers (az_bn3d_stats, the statistics pass of az_bn2d_fwd): the partials merged in fp64 against the fp64 moments
    of the tensor.  Tile t holds voxels v with (v div VPB) mod T = t and shifts by K_t = x[t VPB].  One thread chains
    k = ceil(nvox / (T VPB)) terms (16, or more once T is at its cap of 2048), the block adds VPB - 1 values through LDS:
      e_S(t)  = L1 u sum |x - K_t| + u (|n_t K_t| + |S_t|),         L1 = k + VPB            (the subtraction, the chain, LDS)
      e_M2(t) = L2 u sum (x - K_t)^2 + (2 |s_t| e_s + e_s^2) / n_t + 2 u s_t^2 / n_t + u M2_t,   L2 = k + VPB + 2
    (s_t the shifted sum, e_s its part of e_S); the merged mean may be off by sum_t e_S(t) / N and the merged M2 by
    sum_t [e_M2(t) + 2 |mean_t - mean| e_S(t) + e_S(t)^2 / n_t], all times 1.01 for the second-order terms.  That is check
    (a), sound.  Check (b) is the random walk: L1 and L2 replaced by their square roots, times the constants below.  The counts
    must add up to the voxel count exactly and no M2 partial may be negative.

backward (az_bn3d_bwd, az_bn2d_bwd).  dz = dy [mask], mask = (x sc + sh > 0) in fp64 on the recompute path (the product is
    exact in fp64 and rounding does not move a sign), y > 0 for the saved y otherwise; an element with y == 0 has gradient 0.
    Every element is compared.  xhat = (x - mean) invstd with the fp32 mean and invstd the kernel was given.
      dz_out        bit-equal to dy * mask
      dbeta, dgamma fp64 sums of dz and dz xhat over voxels and groups.  One thread of the reduce pass chains
                    k = ceil(nvox / (2 blocks VPB)) terms in each of its two accumulators; then their sum, log2(64 / (C/4))
                    shuffle steps, 3 adds over the waves, the fp32 rounding of the wave sums in the apply pass's prologue
                    (`wsum`) and of the result: L = k + log2(256 / (C/4)) + 4, and 3 more for dgamma (xhat's two roundings,
                    the product).  (a) gamma_L sum |term|, gamma_L = L u / (1 - L u); (b) the same with sqrt(L), times the
                    constant below.
      coef          (k0, k1, k2) = (gamma invstd, sum dz / nvox, sum dz xhat / nvox) per group: u |k0|; the group's sum
                    bound / nvox + u |k|.
      dx            k0 (dz - k1 - xhat k2): |k0| (3 u |xhat k2| + u |dz - k1| + u |dz - k1 - xhat k2|) + 2 u |dx|
                    + |k0| (|dk1| + |xhat| |dk2|) with dk1, dk2 the (a) bounds of coef, times (1 + 2^-20).
      pre-split dx  (split_out = 1) decoded as tests/test_gpu_conv3d.py's _decode_split does: 2^-21 |dx| + 2^-38 bound, the
                    contract of that test, on top of the fp32 dx bound above (the kernel splits the fp32 dx; against the fp64
                    value the contract alone cannot hold where dz - k1 and xhat k2 cancel); the bound written to the amax
                    array must be >= max |dx| and <= 4 max |dx|.  The contract ALONE is held against the fp32 dx of a launch with
                    split_out = 0 on the same inputs (check_split_vs_fp32), at every size.

The (b) constants are twice the worst ratio of this module's own emulations over the cases of
tests/test_bn_error_model_cpu.py (printed by it); none is fitted to a kernel's output.

Record (not a tolerance): the worst ratios of the kernels on an MI355X over every case of tests/test_gpu_bn_fp64.py are in
GPU_RECORD below (apply 1.000: a correctly rounded fma reaches half an ulp; mean 0.995, invstd 0.999: single roundings; scale 0.920, shift 0.759; the
random-walk checks 0.553 (dbeta), 0.749 (dgamma), 0.703 and 0.868 (merged mean and M2 of the statistics); the pre-split amax
bound at most 2.73 max |dx|, the decode contract alone 0.500).
"""
import math

import torch

U = 2.0 ** -24
# The launch constants below mirror csrc/az_common.h and csrc/az_bn3d.hip.  Only az_bn3d_stats_tiles and the workspace sizes can be
# asked of the library (tests/test_gpu_bn_fp64.py does); the grid caps, the nontemporal threshold and the two-stage threshold are not
# visible through the C ABI: if one changes in the C code, change it here too, or the cases no longer sit where they claim to.
SLACK = 1.0 + 2.0 ** -20
CHANNELS = (32, 64, 128)
PRE_SLICES = 32            # BN_PRE_SLICES
TWO_STAGE_TILES = 4096     # az_bn3d_finalize: two stages from this many tiles on (with scratch)
GRID_CAP = 4096            # az_grid_for
STATS_TILE_CAP = 2048      # az_bn3d_stats_tiles
BWD_PARTIAL_FLOATS = 32768  # BN_BWD_PARTIAL_FLOATS
BWD_APPLY_CAP = 1024       # bn_bwd_apply_grid
NT_BYTES = 256 << 20       # BN_NT_BYTES

# check (b): twice the worst ratio of the emulations against the un-scaled random-walk bound (measured by
# tests/test_bn_error_model_cpu.py::test_the_emulations_pass_every_check, printed there)
CB_STATS_MEAN = 0.804   # measured worst 0.402 (C = 64, nvox = 7, groups 3: one tile, the single roundings of fn * K + s)
CB_STATS_M2 = 0.818     # measured worst 0.409 (C = 64, nvox = 7, groups 3)
CB_BWD_SUM = 1.226      # measured worst 0.613 (dbeta; dgamma 0.577; both C = 64, nvox = 7, groups 3, mask recomputed)

# worst ratio per check over every case of tests/test_gpu_bn_fp64.py on an MI355X (a record of one run)
GPU_RECORD = {"apply": 1.000, "coef": 0.992, "dbeta_a": 0.308, "dbeta_b": 0.553, "dgamma_a": 0.347, "dgamma_b": 0.749, "dx": 0.787,
              "dx_split": 0.433, "dx_split_vs_fp32": 0.500, "dz_bits": 0.0, "invstd": 0.999, "mean": 0.995, "running_mean": 0.704, "running_var": 0.645,
              "scale": 0.920, "shift": 0.759, "split_bound": 0.0, "split_bound_over_max": 2.728, "stats_m2_a": 0.255,
              "stats_m2_b": 0.868, "stats_mean_a": 0.298, "stats_mean_b": 0.703}


# ---- launch arithmetic (csrc/az_bn3d.hip, csrc/az_common.h) ----------------------------------------------------------------
def vpb(C):
    return 256 // (C // 4)


def grid_for(items, block=256):
    return min(max((items + block - 1) // block, 1), GRID_CAP)


def stats_tiles(nvox, C):
    return min(max((nvox + vpb(C) * 16 - 1) // (vpb(C) * 16), 1), STATS_TILE_CAP)


def bwd_cap(C):
    return BWD_PARTIAL_FLOATS // (2 * C)


def bwd_blocks_uncapped(nvox, C):
    return grid_for((nvox + vpb(C) - 1) // vpb(C) * 256)


def bwd_blocks(nvox, C):
    return min(bwd_blocks_uncapped(nvox, C), bwd_cap(C))


def bwd_apply_grid(nvox, C):
    return min(grid_for(nvox * C // 4), BWD_APPLY_CAP)


def apply_trips(nvox, C):
    total4 = nvox * C // 4
    return -(-total4 // (grid_for(total4) * 256))


def nontemporal(nvox, C):
    return nvox * C * 4 >= NT_BYTES


def regimes(nvox, C):
    """the launch regimes a tensor of nvox voxels per group reaches, from the arithmetic above"""
    r = set()
    v = vpb(C)
    if nvox < v and stats_tiles(nvox, C) == 1:
        r.add("one_tile_below_vpb")
    if nvox % v:
        r.add("ragged_block")
    if bwd_blocks_uncapped(nvox, C) >= bwd_cap(C):
        r.add("bwd_reduce_cap")
    if nvox * C // 4 > BWD_APPLY_CAP * 256:
        r.add("bwd_apply_cap")
    if apply_trips(nvox, C) > 1:
        r.add("apply_trips")
    if nvox > STATS_TILE_CAP * 16 * v:
        r.add("stats_tile_cap")
    if nontemporal(nvox, C):
        r.add("nontemporal")
    return r


# ---- ratios -----------------------------------------------------------------------------------------------------------------
def ratio(err, lim):
    """max err / lim; where lim = 0 the error must be 0; a NaN anywhere is inf"""
    err, lim = err.double(), lim.double().expand_as(err)
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    pos = lim > 0
    if bool((err[~pos] != 0).any()):
        return float("inf")
    return float((err[pos] / lim[pos]).max()) if bool(pos.any()) else 0.0


def _gamma(L):
    return L * U / (1.0 - L * U)


def _fma(a, b, c):
    """fp32 fma through fp64 (the product of two floats is exact in fp64)"""
    return (a.double() * b.double() + c.double()).float()


# ---- apply ------------------------------------------------------------------------------------------------------------------
def apply_ref(x, scale, shift, res, relu):
    t = x.double() * scale.double()[:, None, :] + shift.double()[:, None, :]
    y = t if res is None else t + res.double()
    lim = U * t.abs() if res is None else U * t.abs() + U * y.abs()
    return (y.clamp_min(0.0) if relu else y), lim * SLACK


def check_apply(y, x, scale, shift, res, relu):
    ref, lim = apply_ref(x, scale, shift, res, relu)
    return {"apply": ratio((y.double() - ref).abs(), lim)}


# ---- Chan merge and finalize ------------------------------------------------------------------------------------------------
def chan_merge(part, cnt):
    """fp64 merge of partials [.., C, T, 2] with counts [.., T] -> N [..], mean [.., C], M2 [.., C]"""
    p, n = part.double(), cnt.double()[..., None, :]
    N = n.sum(-1)
    mean = p[..., 0].sum(-1) / N
    live = n > 0
    tm = torch.where(live, p[..., 0] / n.clamp_min(1.0), torch.zeros_like(p[..., 0]))
    d = torch.where(live, tm - mean[..., None], torch.zeros_like(tm))
    M2 = (torch.where(live, p[..., 1], torch.zeros_like(tm)) + n * d * d).sum(-1)
    return N[..., 0], mean, M2


def slice_terms(part, cnt):
    """the two-stage path's extra terms for one group: (u sum |S_s| / N on the mean, u sum (M2_s + 2 |d_s| |S_s|) on M2)"""
    T = part.shape[-2]
    per = (T + PRE_SLICES - 1) // PRE_SLICES
    N, mean, _ = chan_merge(part, cnt)
    dm, dM2 = torch.zeros_like(mean), torch.zeros_like(mean)
    for s in range(PRE_SLICES):
        t0, t1 = s * per, min((s + 1) * per, T)
        if t1 <= t0 or float(cnt[t0:t1].sum()) == 0.0:
            continue
        ns, ms, M2s = chan_merge(part[:, t0:t1], cnt[t0:t1])
        Ss = part[:, t0:t1, 0].double().sum(-1)
        dm += U * Ss.abs() / N
        dM2 += U * (M2s + 2.0 * (ms - mean).abs() * Ss.abs())
    return dm, dM2


def finalize_ref(part, cnt, gamma, beta, rm, rv, eps, momentum, two_stage=False):
    """fp64 reference and bound of every output of a finalize over the groups of part [G, C, T, 2], cnt [G, T].
    -> dict name -> (ref, bound); running_* only when rm is given ([C], the values before the call)"""
    G = part.shape[0]
    g64, b64 = gamma.double(), beta.double()
    m = float(torch.tensor(momentum, dtype=torch.float32))
    out = {k: [] for k in ("mean", "invstd", "scale", "shift")}
    lim = {k: [] for k in out}
    rm_ref = rv_ref = rm_lim = rv_lim = None
    if rm is not None:
        rm_ref, rv_ref = rm.double().clone(), rv.double().clone()
        rm_lim, rv_lim = torch.zeros_like(rm_ref), torch.zeros_like(rv_ref)
    for g in range(G):
        N, mu, M2 = chan_merge(part[g], cnt[g])
        dmu, dM2 = slice_terms(part[g], cnt[g]) if two_stage else (torch.zeros_like(mu), torch.zeros_like(mu))
        N = float(N)
        var = M2 / N
        istd = (var + eps).rsqrt()
        e_mu = U * mu.abs() + dmu
        e_is = U * istd + 0.5 * istd ** 3 * (dM2 / N) * 1.01
        sc = g64 * istd
        e_sc = g64.abs() * e_is + U * sc.abs()                      # fl(istd) through e_is, the product
        sh = b64 - mu * sc
        e_sh = mu.abs() * e_sc + sc.abs() * e_mu + U * (mu * sc).abs() + U * sh.abs()  # scale's 2, fl(mu), the product, the sum
        for k, r, e in (("mean", mu, e_mu), ("invstd", istd, e_is), ("scale", sc, e_sc), ("shift", sh, e_sh)):
            out[k].append(r)
            lim[k].append(e * SLACK)
        if rm is not None:
            unb = M2 / (N - 1.0) if N > 1.0 else var
            e_unb = U * unb.abs() + dM2 / max(N - 1.0, 1.0)
            for cur, cl, val, ev in ((rm_ref, rm_lim, mu, e_mu), (rv_ref, rv_lim, unb, e_unb)):
                new = (1.0 - m) * cur + m * val
                cl.copy_(((1.0 - m) * cl + 2.0 * U * ((1.0 - m) * cur).abs() + m * ev + U * (m * val).abs() + U * new.abs()) * SLACK)
                cur.copy_(new)
    res = {k: (torch.stack(out[k]), torch.stack(lim[k])) for k in out}
    if rm is not None:
        res["running_mean"], res["running_var"] = (rm_ref, rm_lim), (rv_ref, rv_lim)
    return res


def check_finalize(got, part, cnt, gamma, beta, rm, rv, eps, momentum, two_stage=False):
    """got: dict of the kernel's outputs under finalize_ref's names (running_* after the call; rm, rv before it)"""
    ref = finalize_ref(part, cnt, gamma, beta, rm, rv, eps, momentum, two_stage)
    return {k: ratio((got[k].double().reshape(r.shape) - r).abs(), e) for k, (r, e) in ref.items()}


# ---- statistics producers ---------------------------------------------------------------------------------------------------
def _tile_sums(v, tile, T):
    out = torch.zeros(T, v.shape[1], dtype=torch.float64, device=v.device)
    return out.index_add_(0, tile, v)


def check_stats(part, cnt, x):
    """part [G, C, T, 2], cnt [G, T] as the kernel wrote them, x [G, nvox, C] -> ratios of checks (a) and (b) on the merged
    mean and M2, inf where the counts or the sign of an M2 partial are wrong"""
    G, V, C = x.shape
    T = part.shape[2]
    v_ = vpb(C)
    if float(cnt.double().sum()) != float(G * V) or bool((cnt.double().sum(-1) != V).any()) or bool((part[..., 1] < 0).any()):
        return {"stats_mean_a": float("inf"), "stats_mean_b": float("inf"), "stats_m2_a": float("inf"), "stats_m2_b": float("inf")}
    k = -(-V // (T * v_))
    idx = torch.arange(V, device=x.device)
    tile = (idx // v_) % T
    out = {}
    worst = {"stats_mean_a": 0.0, "stats_mean_b": 0.0, "stats_m2_a": 0.0, "stats_m2_b": 0.0}
    for g in range(G):
        xg = x[g].double()
        mean = xg.mean(0)
        M2 = ((xg - mean) ** 2).sum(0)
        K = xg[torch.arange(T, device=x.device) * v_]                        # [T, C]
        d = xg - K[tile]
        n = torch.zeros(T, dtype=torch.float64, device=x.device).index_add_(0, tile, torch.ones(V, dtype=torch.float64, device=x.device))[:, None]
        A, Q, s = _tile_sums(d.abs(), tile, T), _tile_sums(d * d, tile, T), _tile_sums(d, tile, T)
        S = s + n * K
        M2t = (Q - s * s / n).clamp_min(0.0)
        dt = (S / n - mean).abs()
        _, gm, gM2 = chan_merge(part[g], cnt[g])
        for tag, L1, L2, cm, cM in (("a", k + v_, k + v_ + 2, 1.0, 1.0),
                                    ("b", math.sqrt(k + v_), math.sqrt(k + v_ + 2), CB_STATS_MEAN, CB_STATS_M2)):
            e_s = L1 * U * A
            e_S = e_s + U * ((n * K).abs() + S.abs())
            e_M2 = L2 * U * Q + (2.0 * s.abs() * e_s + e_s * e_s) / n + 2.0 * U * s * s / n + U * M2t
            lim_mean = 1.01 * e_S.sum(0) / V
            lim_M2 = 1.01 * (e_M2 + 2.0 * dt * e_S + e_S * e_S / n).sum(0)
            worst["stats_mean_" + tag] = max(worst["stats_mean_" + tag], ratio((gm - mean).abs(), cm * lim_mean))
            worst["stats_m2_" + tag] = max(worst["stats_m2_" + tag], ratio((gM2 - M2).abs(), cM * lim_M2))
    out.update(worst)
    return out


# ---- backward ---------------------------------------------------------------------------------------------------------------
def relu_mask(x, scale, shift, y):
    """the mask the kernel must take, from the inputs: recompute path when scale is given, the saved y otherwise"""
    if scale is not None:
        return (x.double() * scale.double()[:, None, :] + shift.double()[:, None, :]) > 0
    return y > 0


def bwd_chain(nvox, C):
    """L of dbeta: roundings one value passes through on its way into the sum"""
    k = -(-nvox // (2 * bwd_blocks(nvox, C) * vpb(C)))
    return k + int(math.log2(256 // (C // 4))) + 4


def bwd_ref(dy, x, mean, invstd, gamma, mask):
    """fp64 references and bounds of az_bn*_bwd for dy, x [G, V, C], mean, invstd [G, C], gamma [C], mask bool or None.
    -> dict name -> (ref, bound (a)), plus "dbeta_b" / "dgamma_b" -> bound (b)"""
    G, V, C = x.shape
    dz = dy.double() if mask is None else dy.double() * mask
    xh = (x.double() - mean.double()[:, None, :]) * invstd.double()[:, None, :]
    t2 = dz * xh
    sa, sb = dz.sum(1), t2.sum(1)                 # [G, C]
    Sa, Sb = dz.abs().sum(1), t2.abs().sum(1)
    del t2
    L = bwd_chain(V, C)
    ea, eb = _gamma(L - 1) * Sa, _gamma(L + 2) * Sb           # per group, before the last rounding
    wa, wb = math.sqrt(L - 1) * U * Sa, math.sqrt(L + 2) * U * Sb
    dbeta, dgamma = sa.sum(0), sb.sum(0)
    res = {"dbeta": (dbeta, (ea.sum(0) + U * dbeta.abs()) * SLACK), "dgamma": (dgamma, (eb.sum(0) + U * dgamma.abs()) * SLACK),
           "dbeta_b": (dbeta, CB_BWD_SUM * (wa.sum(0) + U * dbeta.abs())), "dgamma_b": (dgamma, CB_BWD_SUM * (wb.sum(0) + U * dgamma.abs()))}
    k0 = gamma.double()[None, :] * invstd.double()
    k1, k2 = sa / V, sb / V
    e0, e1, e2 = U * k0.abs(), ea / V + U * k1.abs(), eb / V + U * k2.abs()
    res["coef"] = (torch.stack([k0, k1, k2], -1), torch.stack([e0, e1, e2], -1) * SLACK)
    k0, k1, k2, e0, e1, e2 = (t[:, None, :] for t in (k0, k1, k2, e0, e1, e2))
    a = dz - k1
    xk = xh * k2
    inner = a - xk
    dx = k0 * inner
    lim = k0.abs() * (3.0 * U * xk.abs() + U * a.abs() + U * inner.abs()) + 2.0 * U * dx.abs() + k0.abs() * (e1 + xh.abs() * e2)
    res["dx"] = (dx, lim * SLACK)
    return res


def check_bwd(got, dy, x, mean, invstd, gamma, mask, ref=None):
    """got: dx [G,V,C] (fp32, or the decoded fp64 of a pre-split one with got["split_bound"] the amax-array bound),
    dgamma, dbeta [C], coef [G,C,3], dz (optional).  Every element enters."""
    ref = ref or bwd_ref(dy, x, mean, invstd, gamma, mask)
    out = {}
    for k in ("dbeta", "dgamma", "coef"):
        r, e = ref[k]
        out[k + "_a" if k != "coef" else k] = ratio((got[k].double().reshape(r.shape) - r).abs(), e)
    for k in ("dbeta", "dgamma"):
        r, e = ref[k + "_b"]
        out[k + "_b"] = ratio((got[k].double() - r).abs(), e)
    r, e = ref["dx"]
    if got.get("split_bound") is not None:
        bnd = float(got["split_bound"])
        true = float(r.abs().max())
        out["dx_split"] = ratio((got["dx"].double() - r).abs(), e + 2.0 ** -21 * r.abs() + 2.0 ** -38 * bnd)
        out["split_bound"] = 0.0 if (bnd >= true and bnd <= 4.0 * true) else float("inf")
        out["split_bound_over_max"] = bnd / true if true > 0 else 0.0   # (reported; the assertion is the line above)
    else:
        out["dx"] = ratio((got["dx"].double() - r).abs(), e)
    if got.get("dz") is not None:
        want = dy if mask is None else torch.where(mask, dy, torch.zeros_like(dy))  # (a select: +0, never -0)
        out["dz_bits"] = 0.0 if bool((got["dz"].view(torch.int32) == want.view(torch.int32)).all()) else float("inf")
    return out


PASS_KEYS_EXCLUDED = ("split_bound_over_max",)


def check_split_vs_fp32(decoded, bound, dx32):
    """the decode contract alone, against the fp32 dx a launch with split_out = 0 wrote from the same inputs: the pre-split
    tensor is the split of exactly that value, hi + lo = x up to 2^-22 |x|, and the fp16 subnormal spacing on the scaled value
    (tests/test_gpu_conv3d.py: 2^-21 |dx| + 2^-38 bound)"""
    r = dx32.double()
    return {"dx_split_vs_fp32": ratio((decoded.double() - r).abs(), 2.0 ** -21 * r.abs() + 2.0 ** -38 * float(bound))}


def worst(ratios):
    """the largest ratio of a check dict (reported figures that are no ratios left out)"""
    return max(v for k, v in ratios.items() if k not in PASS_KEYS_EXCLUDED)


def decode_split(t, amax):
    """a pre-split tensor -> fp64 values, as tests/test_gpu_conv3d.py's _decode_split: every 16 bytes = hi(c0) hi(c1) |
    hi(c2) hi(c3) | lo(c0) lo(c1) | lo(c2) lo(c3), scaled by 2^k with 2^k bound in [2^14, 2^15)"""
    a = float(amax[::64].max())
    e = int(math.floor(math.log2(a))) if a > 0 else -127
    k = min(max(14 - e, -126), 127)
    h = t.contiguous().view(torch.int16).view(-1, 8)
    f = h.view(torch.float16).double()
    return ((f[:, :4] + f[:, 4:]) * 2.0 ** (-k)).view(t.shape), a


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def make_inputs(G, V, C, seed, device="cpu"):
    """x, dy, residual [G, V, C], gamma, beta [C].  Channel 0: mean 1e3 std 1 (cancellation in x sc + sh and in every
    unshifted sum); channel 1: constant (variance 0, invstd = eps^-1/2); channel 2: beta so low that the ReLU mask is all
    zero; channel 3: mean 30 std 0.1; the rest zero-mean-ish O(1).  dy ~ 1e-3 with a few 300x spikes and a per-channel
    offset (so mean(dz) is not small)."""
    gen = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(G, V, C, generator=gen, device=device) * 2.0 + 0.5
    x[:, :, 0] = 1e3 + x[:, :, 0] * 0.5
    x[:, :, 1] = -3.25
    x[:, :, 3] = 30.0 + x[:, :, 3] * 0.05
    dy = torch.randn(G, V, C, generator=gen, device=device) * 1e-3
    dy += torch.linspace(-1e-3, 1e-3, C, device=device)
    for i in range(3):
        dy[i % G, (V * (i + 1)) // 5, :] *= 300.0
    res = torch.randn(G, V, C, generator=gen, device=device)
    gamma = (torch.rand(C, generator=gen, device=device) * 1.0 + 0.5)
    beta = (torch.rand(C, generator=gen, device=device) - 0.5)
    beta[2] = -40.0
    gamma[5] = -0.75  # (a negative gamma: the sign of k0)
    return x, dy, res, gamma, beta


def moments32(x, eps):
    """fp32 (mean, invstd) [G, C] of x [G, V, C], rounded from fp64 (inputs of a backward test: any fp32 values would do)"""
    xd = x.double()
    mean = xd.mean(1)
    var = ((xd - mean[:, None, :]) ** 2).mean(1)
    return mean.float(), (var + eps).rsqrt().float()


# ---- fp32 emulations of the documented algorithms (torch, CPU; independent of the HIP code) -------------------------------
def emu_stats(x, mutant=None):
    """(part [G, C, T, 2], cnt [G, T]) as az_bn3d_stats documents them: T = stats_tiles blocks, block t takes voxels
    t VPB + k T VPB + lane, sums about its first voxel, the lanes' sums are added one after the other"""
    G, V, C = x.shape
    v_, T = vpb(C), stats_tiles(V, C)
    stride = T * v_
    k = -(-V // stride)
    xp = torch.zeros(G, k * stride, C)
    xp[:, :V] = x
    valid = (torch.arange(k * stride) < V).view(k, T, v_)
    xp = xp.view(G, k, T, v_, C)
    K = xp[:, 0, :, 0, :]
    s1 = torch.zeros(G, T, v_, C)
    s2 = torch.zeros(G, T, v_, C)
    for i in range(k):
        d = xp[:, i] - K[:, :, None, :]
        m = valid[i][None, :, :, None]
        s1 = torch.where(m, s1 + d, s1)
        s2 = torch.where(m, _fma(d, d, s2), s2)
    S1, S2 = s1[:, :, 0], s2[:, :, 0]
    for j in range(1, v_):
        S1, S2 = S1 + s1[:, :, j], S2 + s2[:, :, j]
    fn = valid.sum((0, 2)).float()                       # [T]
    if mutant == "ragged_full":
        fn = torch.full_like(fn, float(k * v_))
    f = fn[None, :, None]
    part = torch.stack([_fma(f.expand_as(K), K, S1), (S2 - S1 * S1 / f).clamp_min(0.0)], -1).permute(0, 2, 1, 3).contiguous()
    cnt = fn[None].repeat(G, 1)
    if mutant == "tile_dropped":
        part[:, :, T // 2] = 0.0
        cnt[:, T // 2] = 0.0
    return part, cnt


def _merge64(p, n, mutant=None):
    """Chan merge in fp64 as bn_finalize_kernel: p [C, T, 2], n [T] (fp64) -> N, mean [C], M2 [C]"""
    N = n.sum()
    mean = p[:, :, 0].sum(1) / N if float(N) > 0 else torch.zeros(p.shape[0], dtype=torch.float64)
    live = (n > 0)[None, :]
    d = torch.where(live, p[:, :, 0] / n.clamp_min(1.0)[None, :] - mean[:, None], torch.zeros_like(p[:, :, 0]))
    if mutant == "no_delta_term":
        d = torch.zeros_like(d)
    M2 = torch.where(live, p[:, :, 1] + n[None, :] * d * d, torch.zeros_like(d)).sum(1)
    return N, mean, M2


def emu_finalize(part, cnt, gamma, beta, rm, rv, eps, momentum, two_stage=False, mutant=None):
    G, C, T, _ = part.shape
    out = {k: torch.zeros(G, C) for k in ("mean", "invstd", "scale", "shift")}
    rm, rv = (rm.clone(), rv.clone()) if rm is not None else (None, None)
    m32 = torch.tensor(momentum, dtype=torch.float32)
    om32 = torch.tensor(1.0, dtype=torch.float32) - m32
    order = range(G - 1, -1, -1) if mutant == "reverse_groups" else range(G)
    for g in order:
        src = 0 if mutant == "group0_partials" else g
        p, n = part[src].double(), cnt[src].double()
        if two_stage:
            per = (T + PRE_SLICES - 1) // PRE_SLICES
            p2, n2 = torch.zeros(C, PRE_SLICES, 2, dtype=torch.float64), torch.zeros(PRE_SLICES, dtype=torch.float64)
            for s in range(PRE_SLICES):
                t0, t1 = s * per, min((s + 1) * per, T)
                if t1 <= t0 or (mutant == "slice_dropped" and s == 5):
                    continue
                Ns, ms, M2s = _merge64(p[:, t0:t1], n[t0:t1], mutant)
                p2[:, s, 0], p2[:, s, 1], n2[s] = (ms * Ns).float().double(), M2s.float().double(), Ns.float().double()
            p, n = p2, n2
        N, mu, M2 = _merge64(p, n, mutant)
        var = M2 / N
        istd = (var + eps).rsqrt()
        unb = M2 / (N - 1.0) if float(N) > 1.0 else var
        if mutant == "biased_var":
            unb = var
        out["mean"][g], out["invstd"][g] = mu.float(), istd.float()
        sc = gamma * istd.float()
        out["scale"][g], out["shift"][g] = sc, _fma(-mu.float(), sc, beta)
        if rm is not None:
            rm = _fma(om32.expand_as(rm), rm, m32 * mu.float())
            rv = _fma(om32.expand_as(rv), rv, m32 * unb.float())
    if rm is not None:
        out["running_mean"], out["running_var"] = rm, rv
    return out


def emu_apply(x, scale, shift, res, relu, grid=None, mutant=None):
    """y [G, V, C]; `grid` blocks of 256 threads walk the float4s of a group grid-stride (default: az_grid_for)"""
    G, V, C = x.shape
    sc, sh = scale[:, None, :], shift[:, None, :]
    y = (x * sc + sh) if mutant == "mul_add" else _fma(x, sc.expand_as(x), sh.expand_as(x))
    if res is not None:
        y = y + res
    if relu:
        y = y.clamp_min(0.0)
    if mutant == "trip_skipped":
        total4 = V * C // 4
        grid = grid or grid_for(total4)
        trip = (torch.arange(total4) // (grid * 256)).repeat_interleave(4).view(V, C)
        y = torch.where((trip == 1)[None], torch.full_like(y, float("nan")), y)  # (never written: what the buffer held)
    return y


def _tree(a, dim):
    """the xor-shuffle butterfly over `dim` (a power of two): neighbours first"""
    while a.shape[dim] > 1:
        a = a.index_select(dim, torch.arange(0, a.shape[dim], 2)) + a.index_select(dim, torch.arange(1, a.shape[dim], 2))
    return a.squeeze(dim)


def emu_bwd(dy, x, y, mean, invstd, gamma, scale, shift, relu, mutant=None):
    """dict dx, dz, dgamma, dbeta, coef of the two-pass backward: the reduce pass (blocks capped, two accumulators per
    thread, shuffle butterfly, four waves) and the apply pass with the fp64 merge of the block partials in its prologue"""
    G, V, C = x.shape
    v_, blocks = vpb(C), bwd_blocks(V, C)
    stride = blocks * v_
    k = -(-V // stride)
    if relu:
        yy = _fma(x, scale[:, None, :].expand_as(x), shift[:, None, :].expand_as(x)) if scale is not None else y
        mask = (yy >= 0) if mutant == "mask_ge" else (yy > 0)
        g = torch.where(mask, dy, torch.zeros_like(dy))
    else:
        g = dy
    xh = (x - mean[:, None, :]) * invstd[:, None, :]
    w = torch.ones(V)
    if mutant == "tail_twice":
        w[max(V - stride, 0):] = 2.0
    pad = k * stride - V
    gp = torch.cat([g * w[None, :, None], torch.zeros(G, pad, C)], 1).view(G, k, blocks, v_, C)
    xp = torch.cat([xh, torch.zeros(G, pad, C)], 1).view(G, k, blocks, v_, C)
    acc1 = [torch.zeros(G, blocks, v_, C), torch.zeros(G, blocks, v_, C)]
    acc2 = [torch.zeros(G, blocks, v_, C), torch.zeros(G, blocks, v_, C)]
    for i in range(k):
        acc1[i % 2] = acc1[i % 2] + gp[:, i]
        acc2[i % 2] = _fma(gp[:, i], xp[:, i], acc2[i % 2])
    part = []
    for a in (acc1[0] + acc1[1], acc2[0] + acc2[1]):
        a = _tree(a.view(G, blocks, 4, v_ // 4, C), 3)                 # lanes of a wave with the same channel quad
        part.append(((a[:, :, 0] + a[:, :, 1]) + a[:, :, 2]) + a[:, :, 3])   # [G, blocks, C]
    rows = 512 // C
    per_wave = rows // 4
    wave_of = (torch.arange(blocks) % rows) // per_wave
    sums = []
    for p in part:
        ws = torch.zeros(G, 4, C, dtype=torch.float64).index_add_(1, wave_of, p.double()).float().double()
        sums.append((ws[:, 0] + ws[:, 1]) + (ws[:, 2] + ws[:, 3]))     # [G, C] fp64
    sa, sb = sums
    k0 = gamma[None, :] * invstd
    k1, k2 = (sa / V).float(), (sb / V).float()
    if mutant == "k2_other_group":
        k2 = k2.roll(1, 0)
    dbeta = sa.sum(0).float()
    dgamma = (sb[0] if mutant == "dgamma_group0" else sb.sum(0)).float()
    k1a = torch.zeros_like(k1) if mutant == "no_mean_dz" else k1
    dx = k0[:, None, :] * (g - k1a[:, None, :] - xh * k2[:, None, :])
    return {"dx": dx, "dz": g, "dgamma": dgamma, "dbeta": dbeta, "coef": torch.stack([k0, k1, k2], -1)}
