"""fp64 references and element-wise error checks of the RAFT-Stereo ConvGRU update: the one-part 3x3 convolutions
(conv2d_same_kernel<NW, 3, 3, 1, PARTS = 1, STATS = false, H1> of az_conv2d.hip, conv2d_wgrad_kernel<MT, NT, 3, 3, 1, AR = 2 | 3> of
az_conv2d_wgrad.hip), their epilogues and the five gate kernels of az_gru_gates.hip.  Shared by tests/test_gru_error_model_cpu.py
and tests/test_gpu_gru_fp64.py (a helper module, not a conftest); built on tests/_fp64ref.py, whose operators, magnitude sums,
kinds (fwd / dgrad / wgrad with operands p, q) and Geom2d(3, 3, 1) it uses unchanged.

The two one-part arithmetics (ARITHS): every operand is rounded ONCE to 16 bits, the products are accumulated in fp32:
    bf16x1   operand -> bf16(x), round to nearest even                                     (az_conv2d_bf16_fwd, az_conv2d_wgrad_bf16)
    f16x1    operand -> fp16(x 2^k) 2^-k, k = f16_scale_exp(amax) where the launch was     (az_conv2d_h1_fwd, az_conv2d_wgrad_h1)
             given an amax array for that operand, k = 0 where it was given none
round_operand(t, arith, amax) takes the amax as a float or None: the two cases of f16x1 are distinct and explicit.
split_reference() is the fp64 bilinear form of the rounded operands.

The three checks of _fp64ref.check, with the same meaning:
  (a) |got - exact| <= bound_a: the worst case of the arithmetic,
          [(2 eps + eps^2) + n 2^-24] S + (f16x1) 2^-25 (2^-kp sum |q| + 2^-kq sum |p|) (1 + eps),     S = sum_k |p_k q_k|
      * operand rounding: p' = p (1 + d), q' = q (1 + e) with |d|, |e| <= eps, so |p' q' - p q| <= (2 eps + eps^2) |p q|, with
        eps the UNIT ROUNDOFF of the format: 2^-8 for bf16 (8 significand bits), 2^-11 for fp16 (11 bits).  The sweep was
        specified with eps = 2^-9 / 2^-12 (EPS_SPECIFIED), half of that, as a form found sound on nine shapes.  It is not a worst
        case: a single product can be off by 2 * 2^-8 of itself, and a weight gradient of a 1 x 1 image IS a single product --
        the exact arithmetic itself (the split reference, no accumulation at all) lands at 1.55 of that form there
        (tests/test_gru_error_model_cpu.py prints it).  A sound bound needs the unit roundoff, so EPS holds it; every case also
        reports its ratio under the specified form (`check(..., eps=EPS_SPECIFIED[arith])`), which outputs of 16 and more
        products pass with room because their rounding errors do not all agree in sign.
      * accumulation: n = rounding_count(): ONE MFMA per 16-deep block chained into the running accumulator (no block
        temporary in the PARTS = 1 instantiations: `acc[cur] = mfma(a, b, acc[cur])`), at most one more add per block for the
        flushes (the weight gradient's one atomicAdd per workgroup and (image, chunk, row segment) column), plus 3 for the
        output scale, bias and residual.  Forward / input gradient: blocks = 9 cin / 16 exactly; weight gradients: blocks =
        wgrad_blocks_2d(dy) = B H ceil(W / 16), one 16-position block per output row and chunk.
      * f16x1 subnormals: below 2^-14 (after the scale) fp16 rounds to multiples of 2^-24, an ABSOLUTE error of 2^-25 2^-k per
        element, times the other operand's rounded magnitude <= |.| (1 + eps).
  (b) |got - split_reference| <= C[arith] 2^-24 (2 + sqrt(K / 32)) S and
  (c) |got - split_reference| <= C2[arith] 2^-24 sqrt(K sum (p q)^2): the random-walk bounds of the fp32 accumulation.

The constants of (b) and (c) start from the f16x3 ones of _fp64ref.py (C = 2.0, C2 = 3.5: the one-part kernels round at most a
third as often) and are kept where the largest err / bound measured on an MI355X over every case of tests/test_gpu_gru_fp64.py
is at most 0.6.  Measured maxima, check (a) / (b) / (c), per arithmetic, kind and instantiation:
                                      bf16x1 (a)   (b)    (c)       f16x1 (a)   (b)    (c)
    fwd    NW 1 (single slab, LATE)       0.26   0.19   0.40          0.21   0.19   0.35
    fwd    NW 2                           0.13   0.15   0.27          0.12   0.16   0.33
    fwd    NW 3                           0.18   0.18   0.28          0.21   0.18   0.36
    fwd    NW 4 (production pairs too)    0.11   0.15   0.36          0.13   0.15   0.38
    dgrad  NW 1                           0.19   0.14   0.41          0.20   0.16   0.39
    dgrad  NW 2                           0.13   0.15   0.37          0.13   0.13   0.29
    dgrad  NW 3                           0.24   0.13   0.29          0.21   0.14   0.30
    dgrad  NW 4 (production pairs too)    0.15   0.12   0.32          0.11   0.13   0.34
    wgrad  1 x 1 (AR 2 | AR 3)            0.91   0.17   0.18          0.88   0.22   0.24   ((b), (c): (1, 2, 1), two row segments)
    wgrad  1 x 2                          0.84   0.08   0.20          0.80   0.08   0.21
    wgrad  2 x 1                          0.92   0.09   0.24          0.83   0.09   0.23
    wgrad  2 x 2 (64 x 64, production)    0.86   0.15   0.30          0.94   0.34   0.59   ((b), (c): (129, 1, 1), 129 items for 72 blocks)
  (fwd rows include the bias / residual / ReLU, pixel-stride and amax variants; f16x1 dgrad the |dy| <= 2^-22 operands.)  Every
  (b) and (c) is at most 0.6, so both constants stay at their starting values.  Check (a) peaks where an output is ONE product
  (the weight gradients of the 1 x 1 image, the corner taps of (1, 2, 1)): 0.80 - 0.94 of the unit-roundoff bound, i.e. 1.6 - 1.9
  of the specified form; every output of 16 and more products stays below 0.27 (0.53 of the specified form).
  Activations: largest |got - f(y0)| 9.2e-8 (sigmoid), 1.1e-7 (tanh), 1.4e-7 (combine), 0.05 / 0.05 / 0.28 of the allowance, with
  pre-activations up to +-100.  Gates, largest err / (8 2^-24 M): rh 0.125, out 0.24, bwd1 dq_pre 0.30, dz 0.43, dh_acc 0.17,
  bwd2 dr 0.34, dh_acc 0.125, bwd3 0.125; every amax bit-identical to the largest finite magnitude of the output.

Epilogues: act 0 / 1 (none / ReLU) go through check()'s epilogue = (ones, bias, residual, relu), as in _fp64ref.check.  The gate
activations (act 2 sigmoid, 3 tanh, 4 the GRU combine (1 - z) h + z tanh(.)) exist only in these instantiations; they are checked
against the kernel's OWN pre-activation y0 (the act 0 output of the same launch: same instantiation and order, so the bits the
epilogue sees): act_check().  Allowance: 2e-6 (act 4: 2e-6 |z|) for the fast exponential -- the figure
tests/test_gpu_raft_gru.py::test_bf16_conv_exact_on_representable_operands asserts -- plus, for act 4, the four fp32 roundings of
the combine (1 - z, two products, one sum): 4 2^-24 ((1 + |z|) |h| + |z q|).

The gate kernels (az_gru_gates.hip, header comment) have references that return (value, M): the fp64 value and the sum of the
absolute values of the output's expanded monomials.  Every output is a product or a two-term sum of fp32 values; counted
roundings, each relative to a quantity <= M:
    rh     r h                         1                      M = |r h|          (the x half is a copy: M = 0, exact)
    out    (1 - z) h + z q             1 + 1, 1, 1 = 4        M = (1 + |z|) |h| + |z q|
    bwd1   dq_pre = g z (1 - q^2)      q q, 1 - ., g z, * = 4     M = |g z| (1 + q^2)
           dz = g (q - h) z (1 - z)    q - h, 1 - z, 3 products = 5   M = |g z| (|q| + |h|) (1 + |z|)
           dh_acc = g (1 - z)          2                      M = |g| (1 + |z|)
    bwd2   dr = d h r (1 - r)          4                      M = |d h r| (1 + |r|)
           dh_acc += d r               2                      M = |dh_acc| + |d r|
    bwd3   dh = dh_acc + d_hx, dx = d_rhx + d_hx   1          M = |a| + |b|
at most 5 per term and one for the sum: gate_ratio() allows 8 2^-24 M plus the fp32 subnormal spacing 2^-149 (FMA contraction only
lowers the count).  Cancellation (1 - q^2 with |q| -> 1) is covered because M is taken over the expanded monomials.  The amax
arrays bwd1 / bwd2 write are compared BIT FOR BIT with amax_of() of the kernel's own fp32 output (largest finite magnitude).
"""
import math

import torch

from tests import _fp64ref as R

U = R.U
G33 = R.Geom2d(3, 3, 1)
KINDS = R.KINDS
ARITHS = ("bf16x1", "f16x1")
EPS = {"bf16x1": 2.0 ** -8, "f16x1": 2.0 ** -11}            # unit roundoffs: the sound worst case
EPS_SPECIFIED = {"bf16x1": 2.0 ** -9, "f16x1": 2.0 ** -12}  # the form the sweep was specified with (module docstring)
C = {"bf16x1": 2.0, "f16x1": 2.0}
C2 = {"bf16x1": 3.5, "f16x1": 3.5}
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, ACT_GRU = range(5)
EXP_TOL = 2e-6


# ---- the one-part arithmetics ---------------------------------------------------------------------------------------------------
def scale_exp(arith, amax):
    """k of an operand: f16x1 with an amax array -> f16_scale_exp(amax); without one, and for bf16x1 -> 0"""
    return R.f16_scale_exp(amax) if (arith == "f16x1" and amax is not None) else 0


def round_operand(t, arith, amax=None):
    """the value the arithmetic multiplies, as an unscaled fp64 tensor.  amax: None = the launch had no amax array for this
    operand (k = 0: rounded as it is, the way autocast does); a float = the amax the array held"""
    t = t.float()
    if arith == "bf16x1":
        return t.bfloat16().double()
    k = scale_exp(arith, amax)
    return (t * 2.0 ** k).half().double() * 2.0 ** -k


def split_reference(kind, p, q, arith, amax_p=None, amax_q=None, gemm=False, geom=G33):
    """fp64 bilinear form of the rounded operands"""
    f = R.op_gemm if gemm else R.op
    return f(kind, round_operand(p, arith, amax_p).to(p.device), round_operand(q, arith, amax_q).to(q.device), geom)


def rounding_count(K, blocks=None):
    """one MFMA per 16-deep block chained into the accumulator + one flush add per block + 3 (module docstring)"""
    blocks = math.ceil(K / 16) if blocks is None else max(blocks, math.ceil(K / 16))
    return 2 * blocks + 3


def bound_a(arith, K, ex, kp=0, kq=0, blocks=None, eps=None):
    e = EPS[arith] if eps is None else eps
    lim = ((2.0 * e + e * e) + rounding_count(K, blocks) * U) * ex["S"]
    if arith == "f16x1":
        lim = lim + 2.0 ** -25 * (2.0 ** -kp * ex["sum_q"] + 2.0 ** -kq * ex["sum_p"]) * (1.0 + e)
    return lim


def bound_b(arith, K, ex):
    return C[arith] * U * (2.0 + math.sqrt(K / 32.0)) * ex["S"]


def bound_c(arith, K, ex):
    return C2[arith] * U * (K * ex["Q2"]).sqrt()


def check(got, arith, K, ex, sref, amax_p=None, amax_q=None, blocks=None, epilogue=None, eps=None):
    """(ratio a, ratio b, ratio c): the largest err / bound of each check (<= 1 passes), as _fp64ref.check.
    amax_p / amax_q: what the launch's amax arrays held (None: no array); epilogue = (scale [C], shift [C], res or None, relu);
    eps: the operand term of bound (a) with another eps than EPS[arith]"""
    got = got.double().to(ex["y"].device)
    y, sr = ex["y"], sref.to(ex["y"].device)
    la = bound_a(arith, K, ex, scale_exp(arith, amax_p), scale_exp(arith, amax_q), blocks, eps)
    lb, lc = bound_b(arith, K, ex), bound_c(arith, K, ex)
    if epilogue is not None:
        scale, shift, res, relu = epilogue
        bc = (lambda t: t.double().to(y.device).reshape(1, -1, *([1] * (y.dim() - 2))))
        sc, sh = bc(scale), bc(shift)
        r = res.double().to(y.device) if res is not None else torch.zeros_like(y)
        extra = 3.0 * U * ((y * sc).abs() + sh.abs() + r.abs())
        la, lb, lc = la * sc.abs() + extra, lb * sc.abs() + extra, lc * sc.abs() + extra
        y, sr = y * sc + sh + r, sr * sc + sh + r
        if relu:
            y, sr = y.clamp_min(0.0), sr.clamp_min(0.0)
    if not bool(torch.isfinite(got).all()):
        return float("inf"), float("inf"), float("inf")
    eb = (got - sr).abs()
    return R._ratio((got - y).abs(), la), R._ratio(eb, lb), R._ratio(eb, lc)


# ---- the gate activations of the epilogue -----------------------------------------------------------------------------------------
def act_reference(y0, act, z=None, h=None):
    """(fp64 function of the pre-activation y0, allowance) of act 2 / 3 / 4"""
    y0 = y0.double()
    if act == ACT_SIGMOID:
        return torch.sigmoid(y0), torch.full_like(y0, EXP_TOL)
    q = torch.tanh(y0)
    if act == ACT_TANH:
        return q, torch.full_like(y0, EXP_TOL)
    assert act == ACT_GRU
    z, h = z.double(), h.double()
    return (1.0 - z) * h + z * q, EXP_TOL * z.abs() + 4.0 * U * ((1.0 + z.abs()) * h.abs() + (z * q).abs())


def act_check(got, y0, act, z=None, h=None):
    """(largest err / allowance, largest absolute error) of an activated output against the fp64 function of y0"""
    want, lim = act_reference(y0, act, z, h)
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf"), float("inf")
    err = (got - want).abs()
    return R._ratio(err, lim), float(err.max())


# ---- the gate kernels: (fp64 value, M) ----------------------------------------------------------------------------------------------
def _d(*ts):
    return [t.double() for t in ts]


def gru_rh(zr, hx, hid):
    """rhx = [r h | x]"""
    zr, hx = _d(zr, hx)
    out = hx.clone()
    out[:, :hid] = zr[:, hid:] * hx[:, :hid]
    m = torch.zeros_like(out)
    m[:, :hid] = out[:, :hid].abs()
    return out, m


def gru_out(zr, q, hx, hid):
    """h' = (1 - z) h + z q"""
    zr, q, hx = _d(zr, q, hx)
    z, h = zr[:, :hid], hx[:, :hid]
    return (1.0 - z) * h + z * q, (1.0 + z.abs()) * h.abs() + (z * q).abs()


def gru_bwd1(g, zr, q, hx, hid):
    """{dq_pre, dz (the z half of dzr), dh_acc}"""
    g, zr, q, hx = _d(g, zr, q, hx)
    z, h = zr[:, :hid], hx[:, :hid]
    gz = (g * z).abs()
    return {"dq": (g * z * (1.0 - q * q), gz * (1.0 + q * q)),
            "dz": (g * (q - h) * z * (1.0 - z), gz * (q.abs() + h.abs()) * (1.0 + z.abs())),
            "dh_acc": (g * (1.0 - z), g.abs() * (1.0 + z.abs()))}


def gru_bwd2(dh_acc, d_rhx, zr, hx, hid):
    """{dr (the r half of dzr), dh_acc (updated)}"""
    dh_acc, d_rhx, zr, hx = _d(dh_acc, d_rhx, zr, hx)
    r, h, d = zr[:, hid:], hx[:, :hid], d_rhx[:, :hid]
    return {"dr": (d * h * r * (1.0 - r), (d * h * r).abs() * (1.0 + r.abs())),
            "dh_acc": (dh_acc + d * r, dh_acc.abs() + (d * r).abs())}


def gru_bwd3(dh_acc, d_rhx, d_hx, hid):
    """{dh, dx}"""
    dh_acc, d_rhx, d_hx = _d(dh_acc, d_rhx, d_hx)
    return {"dh": (dh_acc + d_hx[:, :hid], dh_acc.abs() + d_hx[:, :hid].abs()),
            "dx": (d_rhx[:, hid:] + d_hx[:, hid:], d_rhx[:, hid:].abs() + d_hx[:, hid:].abs())}


def gate_ratio(got, ref):
    """largest err / (8 2^-24 M + 2^-149) of a gate output against its (value, M); where M = 0 and the value is finite (a copy, a
    product with a zero factor) the output must be exact"""
    want, m = ref
    got = got.double().to(want.device)
    fin = torch.isfinite(want)
    if not bool((torch.isfinite(got) == fin).all()):
        return float("inf")
    err = (got[fin] - want[fin]).abs()
    lim = 8.0 * U * m[fin] + 2.0 ** -149 * (m[fin] > 0)
    return R._ratio(err, lim)
