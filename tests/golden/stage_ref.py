"""Stage-rounded fp64 references for the fused kernels of the plain-bf16 ('bf16') contraction mode (pure torch, CPU or GPU).

In this mode the fused kernels share one pattern: the fp32 value entering each MFMA is rounded ONCE to bf16 (the `(__bf16)` casts of
csrc/token_mlp.hip, naf_fused.hip, naf_tail_kernel.inc, naf_front_kernel.inc, sgfn_tail.hip and token_linear.hip), the weights are the
prepared hi plane, and everything else -- LayerNorm, bias, GELU, gate products, kmul / sca scaling before the cast, depth-wise taps,
residuals, output scales -- is fp32.  Each reference below evaluates its kernel's formula in fp64 and applies lowprec_ref.bf16_rne at
exactly the kernel's cast sites (named in a comment at every call of round_point) and nowhere else.

Flip accounting.  A kernel's intermediate can legitimately land on the other side of a bf16 rounding boundary when fp32 noise moves
it.  Every reference therefore carries, next to each fp64 value v, two non-negative bounds computed from the reference alone:
    noise  the fp32 error of the arithmetic that produced v since the last rounding point;
    move   how far v can differ because elements of EARLIER rounding points rounded the other way.
At a rounding point delta = noise + move; an element is fragile when bf16_rne(v - delta) != bf16_rne(v + delta), its possible movement
is the difference of those two roundings (bf16_rne is monotone, so a kernel value anywhere in [v - delta, v + delta] rounds inside that
span; the fp64 -> fp32 -> bf16 double rounding of the reference itself is inside it too), and behind the rounding point noise starts
again at zero while move is that difference.  Movements travel forward in absolute value: through a GEMM as move @ |w|^T, through a
pointwise function by its largest slope, through a product h1 * h2 as |h2| m1 + |h1| m2 + m1 m2.  The movement that reaches an output is
its allowance, and the assertion is per element:
    |out - ref| <= FP32_CHAIN_TOL * max(1, max|ref|) + allow
(noise that reaches an output is NOT added: that is what the fp32 bound is for).

Branching on the LayerNorm operand.  One fragile element of a row's LayerNorm output moves the row's WHOLE hidden vector, a good part of
which then sits near a rounding boundary of the second rounding point: propagated as a movement it makes every output of the row wide,
and with K = 180 operand elements per row, at the noise bound below, that is one row in ten (token_mlp) to one in two (token_projmlp,
whose LayerNorm input carries a GEMM's noise).  But such an element has only TWO possible values.  In the row kernels (token_mlp,
token_projmlp, naf_ffn, naf_tail) the reference therefore enumerates them: per row the LN_BRANCH fragile operand elements with the
largest movement (those whose delta is below 2^-10 |v|, so that exactly one boundary lies inside v +- delta) are set to their lower and
their upper value in all 2^LN_BRANCH combinations, each combination is carried through the rest of the chain as a reference of its own
(variant), with no movement from those elements, and a row of the kernel's output has to agree with ONE variant in every element.  What
is left -- fragile elements beyond the first LN_BRANCH of a row, or too small to have two clean candidates -- is propagated as
movement.  This is exact where the propagation is a bound, so it only narrows what a row may be.

allowance_shares / assert_caps keep the allowance from becoming the hole: at most 10 % of a case's outputs may have
allow > 10 * FP32_CHAIN_TOL * max(1, max|ref|), and no row may have every output above that level unless a fragile element of its
LayerNorm operand was left to propagation (such a row moves its whole hidden vector), which at most 1 row in 20 may do.  Every variant's
rows count as rows.

Constants.  The two noise factors (GEMM_NOISE_C, LN_NOISE_C) are the only MEASURED ones.  Next to them stand rounding budgets of the
pointwise arithmetic between a GEMM and the next cast, counted instruction by instruction in the kernel's source and stated where they
are used; they are upper counts of 2^-24 roundings, small against the GEMM term they are added to, and none was fitted to an output:
    gelu_erf      ff_gelu_fast: 6 on |v| (12 on erf, halved) + 2 on |g|, plus half of the approximation's 1.5e-7
    gelu_tanh     ff_gelu_sig2: 6 + 3.5 |z| on |g|
    gated gate    token_linear.hip:132-134: (hidden + 2) on sum |gw2 gelu| + |gb2|; 6 on sm; 2 on the mix's two products
    naf gate      1 on the product ha * hb; naf_tail's y: 2 on beta * conv3 and 1 on the sum
    projmlp x1    token_mlp.hip:782-789: 2 on |x| + |c2 scale|, 1 on the sum
    sgfn_tail     sgfn_tail.hip:125, :167-178: 13 (3 per normalised value, 9 taps, 1 product), taken as 16
GELU_SLOPE = 1.13 is max |GELU'|.  The branching adds LN_BRANCH = 3 (how many elements are enumerated: cost only, more is tighter) and
the 2^-10 |v| cleanliness threshold (from the bf16 spacing, see branch_round_point).

Covered elsewhere: the attention kernels of this mode (window_attn_bf16s, ocab_attn, win_attn_fused) round softmax probabilities relative
to a running maximum; their flip model is tests/golden/attn_ref.py (which imports this module's accounting), checked on the CPU by
tests/test_attn_ref_cpu.py and held against the kernels by tests/test_lowprec_attn_gpu.py -- win_attn_fused there on fixed-point inputs
that make its LayerNorm and projections exact.  chan_qkv, whose reduction spans the whole image, and the fp32 ff_chan_attn_weights are held per
partial block to tests/golden/chan_ref.py by tests/test_chan_attn_gpu.py.  What remains on the checks of tests/test_ops_gpu.py:
win_attn_fused on generic inputs (a flip model through LayerNorm, projection and softmax together).  The `_images` and
batched forms are pinned bit for bit against the single-image forms by tests/test_batched_*_gpu.py.

tests/test_stage_ref_cpu.py checks this module against fp32 stand-ins (and mutants of them) on the CPU; tests/test_lowprec_fused_gpu.py
holds the kernels to it."""
import math
from collections import namedtuple

import torch

from lowprec_ref import FP32_CHAIN_TOL, act_f64, bf16_rne, layernorm_f64, operand_a, operand_w

U24 = 2.0 ** -24             # half an fp32 ulp of a value in [1, 2): the unit of every noise bound below

# The fp32 error of a length-K dot product of exact products, as a multiple of 2^-24 * (sum_k |a_k||w_k| + |bias|).
# MEASURED is the largest |stand-in - fp64| / (2^-24 * (sum|a||w| + |bias|)) over every GEMM stage of every case of CASES, the stand-in
# being lowprec_ref.chunked_fp32_matmul on the same rounded operands (tests/test_stage_ref_cpu.py repeats the measurement and asserts it
# stays within the constant).  The kernels are held to FOUR times that: the MFMA's summation order and internal width differ from
# ATen's, while both are fp32 sums of the same K exact products.  Neither number was tuned on a kernel's output.
GEMM_NOISE_MEASURED = 2.1
GEMM_NOISE_FACTOR = 4.0
GEMM_NOISE_C = GEMM_NOISE_FACTOR * GEMM_NOISE_MEASURED
# The LayerNorm counterpart: the fp32 error of (x - mean) * rstd * gamma + beta as a multiple of 2^-24 * max(1, |v|), measured the same
# way (two-pass fp32 LayerNorm, the kernels' form, against layernorm_f64) and widened by the same factor for the same reason: the
# kernels sum the row in fragment order with a cross-lane step, ATen sums it as it likes.
LN_NOISE_MEASURED = 4.9
LN_NOISE_C = GEMM_NOISE_FACTOR * LN_NOISE_MEASURED
GELU_SLOPE = 1.13            # max |GELU'| (erf and tanh forms alike: 1.129 at x = 1.41)

WIDE_LEVEL = 10.0            # an allowance is "wide" above WIDE_LEVEL * FP32_CHAIN_TOL * max(1, max|ref|)
WIDE_SHARE_CAP = 0.10        # cap one: share of a case's outputs with a wide allowance
LN_ROW_SHARE_CAP = 0.05      # cap two: share of rows that are wide throughout BECAUSE their LayerNorm operand is fragile (no other row may be)

LN_BRANCH = 3                # fragile LayerNorm operand elements per row that are enumerated instead of propagated (8 variants)

StageRef = namedtuple("StageRef", "ref allow shape ln_rows gemms lns")
# ref, allow: fp64 [variants, rows, outputs per row] (variant 0 = every operand at its nominal rounding; one variant where the kernel
# is not branched).  shape: the kernel output's shape.  ln_rows: bool [variants, rows], the rows in which a fragile LayerNorm operand
# element is left to propagation (None: no LayerNorm).  gemms: [(a fp64, w fp64, bias or None)] every GEMM stage's operands (all
# variants' rows); lns: [(x fp64, gamma, beta, eps)] every LayerNorm's -- what the CPU test measures the two noise constants on.


# ---------------------------------------------------------------------------------------------------------------------
# the accounting
def round_point(v: torch.Tensor, delta: torch.Tensor):
    """fp64 v, delta >= 0 -> (bf16_rne(v) as fp64, movement >= 0): the reference operand and how far a kernel value within delta of v
    can round away from it."""
    assert v.dtype == torch.float64
    lo = bf16_rne((v - delta).float()).double()
    hi = bf16_rne((v + delta).float()).double()
    return bf16_rne(v.float()).double(), hi - lo


def branch_round_point(v: torch.Tensor, delta: torch.Tensor, nb: int = LN_BRANCH):
    """round_point for a LayerNorm operand v [M, K] with the nb largest clean fragile elements of every row enumerated:
    -> (a [2^nb * M, K], movement of the elements left to propagation [2^nb * M, K], row index [2^nb * M] into the M rows);
    variant j occupies rows j M .. (j + 1) M - 1, variant 0 is round_point's own operand."""
    M = v.shape[0]
    lo = bf16_rne((v - delta).float()).double()
    hi = bf16_rne((v + delta).float()).double()
    a0, mv = bf16_rne(v.float()).double(), hi - lo
    clean = (mv > 0) & (delta < v.abs() * 2.0 ** -10)          # bf16 spacing around v is >= 2^-9 |v|: one boundary inside v +- delta
    vals, idx = torch.where(clean, mv, torch.zeros_like(mv)).topk(nb, dim=-1)
    act = vals > 0
    rows = torch.arange(M, device=v.device)
    a_all, m_all = [], []
    for j in range(2 ** nb):
        a, m = a0.clone(), mv.clone()
        for f in range(nb):
            r, c = rows[act[:, f]], idx[act[:, f], f]
            nominal_is_hi = a0[r, c] == hi[r, c]
            flip = bool((j >> f) & 1)                          # bit f of j set: the candidate that is NOT the nominal rounding
            a[r, c] = torch.where(nominal_is_hi != flip, hi[r, c], lo[r, c])
            m[r, c] = 0.0
        a_all.append(a)
        m_all.append(m)
    return torch.cat(a_all), torch.cat(m_all), rows.repeat(2 ** nb)


def gemm(a, move, w, bias, log):
    """a [M, K] fp64 (bf16 values), w [N, K] fp32 weights (rounded to the hi plane here), bias fp32 or None
    -> (y, noise, move) of y = a @ w^T + bias."""
    w64 = operand_w(w)
    y = a.matmul(w64.t())
    mag = a.abs().matmul(w64.abs().t())
    if bias is not None:
        y = y + bias.double()
        mag = mag + bias.double().abs()
    log.append((a, w64, bias))
    mv = torch.zeros_like(y) if move is None else move.matmul(w64.abs().t())
    return y, GEMM_NOISE_C * U24 * mag, mv


def ln_noise(v):
    return LN_NOISE_C * U24 * v.abs().clamp_min(1.0)


def ln_dev(x, d, gamma, eps):
    """First-order bound on how far LayerNorm(x) * gamma + beta moves when x moves by at most d per element (x, d fp64 [M, K]):
    d v_k = gamma_k (rstd (dx_k - dmean) + (x_k - mean) drstd), |dmean| <= mean(d), |drstd| <= rstd^3 mean(|x - mean| d)."""
    xc = x - x.mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(xc.pow(2).mean(-1, keepdim=True) + eps)
    dr = r.pow(3) * (xc.abs() * d).mean(-1, keepdim=True)
    return gamma.double().abs() * (r * (d + d.mean(-1, keepdim=True)) + xc.abs() * dr)


def prod_dev(a, b, da, db):
    return b.abs() * da + a.abs() * db + da * db


def gelu_erf(v, noise, move):
    """ff_gelu_fast: the erf form (Abramowitz-Stegun 7.1.26, |erf error| <= 1.5e-7) -- five fma, rcp, exp2 and four multiplies on values
    <= 1.5, about 12 roundings of 2^-24 on erf, halved and scaled by |v|, plus the two roundings of the result."""
    g = act_f64(v, "gelu", "erf")
    return g, GELU_SLOPE * noise + v.abs() * (0.75e-7 + 6 * U24) + 2 * U24 * g.abs(), GELU_SLOPE * move


def gelu_tanh(v, noise, move):
    """ff_gelu_sig2: x * sigmoid(2u) = the tanh form.  z = x (B x^2 + A) carries three roundings and the two rounded constants
    (5 * 2^-24 |z|, which exp2 turns into a relative error of ln2 * that), exp2 and rcp one ulp (2 * 2^-24) each, the add and the last
    multiply one rounding each; the sigmoid's relative error is at most that of e."""
    g = act_f64(v, "gelu", "tanh")
    z = 2.0 * math.sqrt(2.0 / math.pi) * v.abs() * (1.0 + 0.044715 * v * v)
    return g, GELU_SLOPE * noise + (6.0 + 3.5 * z) * U24 * g.abs(), GELU_SLOPE * move


def _variants(ref, allow, m1, shape, gm, lns):
    """Rows [variants * M, N] of a branched chain -> StageRef."""
    M = shape[0]
    return StageRef(ref.reshape(-1, M, ref.shape[-1]), allow.reshape(-1, M, ref.shape[-1]), tuple(shape), (m1 > 0).any(-1).reshape(-1, M), gm, lns)


def _single(ref, allow, shape, gm):
    return StageRef(ref.reshape(1, -1, ref.shape[-1]), allow.reshape(1, -1, ref.shape[-1]), tuple(shape), None, gm, [])


# ---------------------------------------------------------------------------------------------------------------------
# the references
def token_mlp_ref(x, gamma, beta, w1, b1, w2, b2, eps=1e-5):
    """ops.token_mlp: x + fc2(GELU(fc1(LayerNorm(x)))), GELU = ff_gelu_fast (token_mlp.hip:173)."""
    gm, lns = [], [(x.double(), gamma, beta, eps)]
    v = layernorm_f64(x, gamma, beta, eps)
    a1, m1, ri = branch_round_point(v, ln_noise(v))            # token_mlp.hip:114 (ff_bf16_split, ff_common.h:216): h = (__bf16)f
    h, nz, mv = gemm(a1, m1, w1, b1, gm)
    g, nz, mv = gelu_erf(h, nz, mv)
    a2, m2 = round_point(g, nz + mv)                           # token_mlp.hip:174: h = (__bf16)g
    o, _, allow = gemm(a2, m2, w2, b2, gm)
    return _variants(x.double()[ri] + o, allow, m1, x.shape, gm, lns)


def token_projmlp_ref(att, x, wp, bp, w1, b1, w2, b2, gamma, beta, c2=None, c2_scale=None, eps=1e-5):
    """ops.token_projmlp (token_projmlp_bf16_kernel): x1 = x + proj(att) + c2 * c2_scale; x1 + fc2(GELU(fc1(LayerNorm(x1)))), GELU =
    ff_gelu_sig2 (token_mlp.hip:865).  att / c2 may be bf16 rows: they are then exact operands (token_mlp.hip:702, :738)."""
    gm = []
    a0 = att.double() if att.dtype == torch.bfloat16 else bf16_rne(att).double()       # token_mlp.hip:715: xh = (__bf16)v -- an exact input, no noise
    p, nz_p, _ = gemm(a0, None, wp, bp, gm)
    r0 = x.double()
    mag = r0.abs()
    if c2 is not None:
        t = c2.double() * c2_scale.double()                    # token_mlp.hip:782: r0 += rc * sc (fp32; c2 bf16 rows upcast exactly)
        r0 = r0 + t
        mag = mag + t.abs()
    x1 = p + r0
    nz1 = nz_p + 2 * U24 * mag + U24 * x1.abs()
    lns = [(x1, gamma, beta, eps)]
    v = layernorm_f64(x1, gamma, beta, eps)
    a1, m1, ri = branch_round_point(v, ln_noise(v) + ln_dev(x1, nz1, gamma, eps))     # token_mlp.hip:827: xh = (__bf16)((oacc - mean) * rstd * g4 + b4)
    h, nz, mv = gemm(a1, m1, w1, b1, gm)
    g, nz, mv = gelu_tanh(h, nz, mv)
    a2, m2 = round_point(g, nz + mv)                           # token_mlp.hip:866-867: gh = (__bf16)g[0], (__bf16)g[1]
    o, _, allow = gemm(a2, m2, w2, b2, gm)
    return _variants(x1[ri] + o, allow, m1, x.shape, gm, lns)


def token_linear_gated_ref(x, x2, cm, gw1, gb1, gw2, gb2, w, b, res=None):
    """ops.token_linear_gated: res + W (x * cm + x2 * sm) + b, sm = sigmoid(gw2 . gelu(GW1 x + gb1) + gb2), gelu = ff_gelu_fast
    (token_linear.hip:132), gw2 in fp32."""
    gm = []
    a0 = bf16_rne(x).double()                                  # token_linear.hip:98: h = (__bf16)v -- an exact input, no noise
    ga, nz, _ = gemm(a0, None, gw1, gb1, gm)
    ge, nz, _ = gelu_erf(ga, nz, torch.zeros_like(ga))
    w2d = gw2.double().reshape(1, -1)
    terms = ge.abs().matmul(w2d.abs().t())
    sacc = ge.matmul(w2d.t()) + float(torch.tensor(gb2, dtype=torch.float32))
    nz_s = nz.matmul(w2d.abs().t()) + (w2d.shape[1] + 2) * U24 * (terms + abs(gb2))     # 32 fma + one cross-lane add + gb2
    sm = torch.sigmoid(sacc)                                   # [M, 1]
    nz_sm = 0.25 * nz_s + 6 * U24 * sm                         # sigmoid slope <= 1/4; expf (2 ulp), the add, the division
    sc, oc = x.double() * cm.double(), x2.double() * sm
    mix = sc + oc
    nz_mix = x2.double().abs() * nz_sm + 2 * U24 * (sc.abs() + oc.abs())
    a1, m1 = round_point(mix, nz_mix)                          # token_linear.hip:174: h = (__bf16)f, f = sv * cmv + o * sm
    o, _, allow = gemm(a1, m1, w, b, gm)
    if res is not None:
        o = o + res.double()
    return _single(o, allow, o.shape, gm)


def _naf_ffn_chain(y, nz_y, w4, b4, w5, b5, ln_g, ln_b, oscale, eps, gm):
    """The gated FFN both NAFNet kernels end in; its two rounding points are named by the callers."""
    C = y.shape[-1]
    lns = [(y, ln_g, ln_b, eps)]
    v = layernorm_f64(y, ln_g, ln_b, eps)
    d = ln_noise(v) if nz_y is None else ln_noise(v) + ln_dev(y, nz_y, ln_g, eps)
    a1, m1, ri = branch_round_point(v, d)                      # naf_fused.hip:182 / naf_tail_kernel.inc:176: (__bf16)f, the LayerNorm output
    h, nz, mv = gemm(a1, m1, w4, b4, gm)
    ha, hb = h[:, :C], h[:, C:]
    gt = ha * hb
    nz_g = prod_dev(ha, hb, nz[:, :C], nz[:, C:]) + U24 * gt.abs()
    mv_g = prod_dev(ha, hb, mv[:, :C], mv[:, C:])
    a2, m2 = round_point(gt, nz_g + mv_g)                      # naf_fused.hip:237 / naf_tail_kernel.inc:207: (__bf16)(ha * hb), the gate product
    acc, _, mv_o = gemm(a2, m2, w5, b5, gm)                    # naf_fused.hip:279 / naf_tail_kernel.inc:232: (acc + b5) * scale + y
    return _variants(y[ri] + oscale.double() * acc, oscale.double().abs() * mv_o, m1, y.shape, gm, lns)


def naf_ffn_ref(y, w4, b4, w5, b5, ln_g, ln_b, oscale, eps=1e-6):
    """ops.naf_ffn: y + out_scale * conv5(SimpleGate(conv4(LayerNorm(y)))).
    Rounding points: naf_fused.hip:182 (h = (__bf16)f, the LayerNorm output) and :237 (h = (__bf16)gt, the gate product)."""
    return _naf_ffn_chain(y.double(), None, w4, b4, w5, b5, ln_g, ln_b, oscale, eps, [])


def naf_tail_ref(g, x, w3, b3, w4, b4, w5, b5, sca, beta, ln_g, ln_b, gamma, eps=1e-6):
    """ops.naf_tail: y = x + beta * conv3(g * sca), then naf_ffn on y.
    Rounding points: naf_tail_kernel.inc:103 (gb = (__bf16)(a * s0): ONE fp32 multiply of two exact inputs, which operand_a repeats
    bit for bit -- no noise, so never fragile), :176 (xh = (__bf16)f, the LayerNorm output) and :207 (gh = (__bf16)(ha * hb))."""
    gm = []
    a0 = operand_a(g, "bf16", sca)                             # naf_tail_kernel.inc:103
    c3, nz, _ = gemm(a0, None, w3, b3, gm)
    t = beta.double() * c3
    y = x.double() + t                                         # naf_tail_kernel.inc:132, :141: (acc + b3) * beta + x
    nz_y = beta.double().abs() * nz + 2 * U24 * t.abs() + U24 * y.abs()
    return _naf_ffn_chain(y, nz_y, w4, b4, w5, b5, ln_g, ln_b, gamma, eps, gm)


def _dw3x3(t, wt):
    """Depth-wise 3x3, zero padding, on [H, W, C] fp64 with tap-major weights wt [9, C] fp64 (cross-correlation, as nn.Conv2d)."""
    H, W, _ = t.shape
    tp = torch.nn.functional.pad(t, (0, 0, 1, 1, 1, 1))
    out = torch.zeros_like(t)
    for ky in range(3):
        for kx in range(3):
            out = out + tp[ky:ky + H, kx:kx + W, :] * wt[3 * ky + kx]
    return out


def naf_front_ref(x, w1, b1, ln_g, ln_b, wdw, bdw, eps=1e-6):
    """ops.naf_front on x [1, H, W, C]: SimpleGate(dw3x3(conv1(LayerNorm2d(x)))) and its mean over the pixels.  wdw [2C, 1, 3, 3].
    One rounding point, naf_front_kernel.inc:126 (h = (__bf16)f, the LayerNorm output); conv1's output is zero outside the image
    (:162) and stays fp32 through the taps and the gate.  Returns (gated StageRef, pooled StageRef)."""
    _, H, W, C = x.shape
    gm = []
    xr = x.double().reshape(H * W, C)
    lns = [(xr, ln_g, ln_b, eps)]
    v = layernorm_f64(xr, ln_g, ln_b, eps)
    a1, m1 = round_point(v, ln_noise(v))                       # naf_front_kernel.inc:126
    t, _, mv = gemm(a1, m1, w1, b1, gm)
    wt = wdw.double().reshape(2 * C, 9).t()
    d = _dw3x3(t.reshape(H, W, 2 * C), wt) + bdw.double()
    md = _dw3x3(mv.reshape(H, W, 2 * C), wt.abs())
    gate = d[..., :C] * d[..., C:]
    allow = prod_dev(d[..., :C], d[..., C:], md[..., :C], md[..., C:])
    frag = (m1 > 0).any(-1).reshape(1, 1, H, W).double()
    lr = torch.nn.functional.max_pool2d(frag, 3, 1, 1).reshape(-1) > 0          # a fragile pixel reaches its 3x3 neighbourhood
    return (StageRef(gate.reshape(1, H * W, C), allow.reshape(1, H * W, C), (1, H, W, C), lr.reshape(1, -1), gm, lns),
            StageRef(gate.mean(dim=(0, 1)).reshape(1, 1, C), allow.mean(dim=(0, 1)).reshape(1, 1, C), (1, C), None, gm, lns))


def sgfn_tail_ref(y, c2, wd, bd, stats, gamma, beta, w2, b2, res=None):
    """ops.sgfn_tail on y [1, H, W, >= 2 c2]: res + fc2(y[..., :c2] * (dw3x3(LayerNorm(y[..., c2:2 c2])) + bd)) + b2, the LayerNorm from
    the GIVEN fp32 (mean, rstd) of `stats` (exact inputs here), zero padding after the normalisation.  wd [c2, 1, 3, 3].
    One rounding point, sgfn_tail.hip:181 (g = (__bf16)ga, the gate product).  Its noise: a normalised value carries three roundings, the
    nine taps nine more on the running sum, the product with x1 one: 13 roundings of 2^-24 on |x1| (sum |xn||w| + |bd|), taken as 16."""
    _, H, W, _ = y.shape
    gm = []
    yd = y.double()
    x1, x2 = yd[0, :, :, :c2], yd[0, :, :, c2:2 * c2]
    st = stats.double().reshape(H, W, 2)
    xn = (x2 - st[..., 0:1]) * st[..., 1:2] * gamma.double() + beta.double()       # sgfn_tail.hip:125
    wt = wd.double().reshape(c2, 9).t()
    bdd = torch.zeros(c2, dtype=torch.float64, device=y.device) if bd is None else bd.double()
    conv = _dw3x3(xn, wt) + bdd
    mag = _dw3x3(xn.abs(), wt.abs()) + bdd.abs()
    gate = (x1 * conv).reshape(H * W, c2)
    nz = (16 * U24 * x1.abs() * mag).reshape(H * W, c2)
    a1, m1 = round_point(gate, nz)                             # sgfn_tail.hip:181
    o, _, allow = gemm(a1, m1, w2, b2, gm)
    if res is not None:
        o = o + res.double().reshape(H * W, -1)
    return _single(o, allow, (1, H, W, w2.shape[0]), gm)


# ---------------------------------------------------------------------------------------------------------------------
# the assertion and the two caps
def compare(out, sr: StageRef):
    """-> (err, excess), both as fractions of max(1, max|ref|) (of variant 0).  Per row the variant is taken whose worst
    |out - ref| - allow is smallest: the row has to agree with ONE variant in every element.  excess is the largest of those over the
    rows, err the largest |out - ref| against the variants so chosen.  The assertion of this module is excess <= FP32_CHAIN_TOL.
    (No case has a bf16 output row; one that does adds the half-ulp term of lowprec_ref.bf16_row_excess.)"""
    assert tuple(out.shape) == sr.shape, (tuple(out.shape), sr.shape)
    ref = sr.ref
    scale = max(1.0, ref[0].abs().max().item())
    d = (out.double().to(ref.device).reshape(1, ref.shape[1], ref.shape[2]) - ref).abs()
    exc, pick = (d - sr.allow).max(-1).values.min(0)           # [rows]
    err = d.max(-1).values.gather(0, pick.reshape(1, -1))
    return err.max().item() / scale, exc.max().item() / scale


def allowance_shares(sr: StageRef) -> dict:
    """From the reference alone, every variant's rows counted as rows: wide = share of outputs whose allowance exceeds
    WIDE_LEVEL * FP32_CHAIN_TOL * max(1, max|ref|); rows_unexplained = number of rows wide throughout in which NO fragile LayerNorm
    element was left to propagation (must be 0); rows_ln = share of rows wide throughout in which one was."""
    level = WIDE_LEVEL * FP32_CHAIN_TOL * max(1.0, sr.ref[0].abs().max().item())
    wide = sr.allow > level
    full = wide.all(-1)
    ln = sr.ln_rows if sr.ln_rows is not None else torch.zeros_like(full)
    return dict(wide=wide.double().mean().item(), rows_unexplained=int((full & ~ln).sum().item()),
                rows_ln=(full & ln).double().mean().item(), fragile_ln_rows=ln.double().mean().item())


def assert_caps(sr: StageRef, name: str) -> dict:
    s = allowance_shares(sr)
    print(f"STAGE_REF_SHARES {name}: wide allowances {s['wide']:.4f} of the outputs (cap {WIDE_SHARE_CAP}), rows wide throughout: "
          f"{s['rows_unexplained']} unexplained (cap 0), {s['rows_ln']:.4f} behind a fragile LayerNorm element (cap {LN_ROW_SHARE_CAP}; "
          f"{s['fragile_ln_rows']:.4f} of the rows have one)")
    assert s["wide"] <= WIDE_SHARE_CAP, (name, s)
    assert s["rows_unexplained"] == 0, (name, s)
    assert s["rows_ln"] <= LN_ROW_SHARE_CAP, (name, s)
    return s


# ---------------------------------------------------------------------------------------------------------------------
# the case table (shared by the CPU and the GPU test) and its inputs: activations randn * 1.5 + 0.3, weights randn / sqrt(K),
# non-trivial gamma / beta / bias, scales that are not powers of two.  CPU tensors; the GPU test moves them.
def rnd(*shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _lin(n, k, seed):
    return rnd(n, k, seed=seed, scale=1.0 / math.sqrt(k)), rnd(n, seed=seed + 1, scale=0.1)


def _ln(c, seed):
    return rnd(c, seed=seed) * 0.1 + 1, rnd(c, seed=seed + 1) * 0.1


CASES = {
    # token kernels: 32 rows per wave, 256 per workgroup -- a partial wave in the only workgroup; a full workgroup plus a partial one
    "token_mlp": [dict(M=77), dict(M=293)],
    "token_projmlp": [dict(M=M, c2=c2, io=io) for M in (77, 293) for c2, io in ((False, 0), (True, 0), (True, 1), (True, 2), (True, 3))],
    "token_linear_gated": [dict(M=77), dict(M=293)],
    # 128-row tiles, a partial tile last
    "naf_ffn": [dict(C=C, M=M) for C in (64, 128) for M in (77, 300)],
    "naf_tail": [dict(C=C, M=M, views=False) for C in (64, 128) for M in (77, 300)] + [dict(C=64, M=300, views=True), dict(C=128, M=77, views=True)],
    # partial 8 x 16 tiles on both edges
    "naf_front": [dict(C=C, H=H, W=W) for C in (64, 128) for H, W in ((9, 17), (20, 40))],
    "sgfn_tail": [dict(H=H, W=W, res=r) for H, W in ((8, 32), (19, 70)) for r in (True, False)],
}


def case_name(case: dict) -> str:
    return " ".join(f"{k}={v}" for k, v in case.items())


def make_inputs(kernel: str, case: dict) -> dict:
    """The reference's keyword arguments for one case (fp32 CPU tensors; bf16 rows where the case has them)."""
    if kernel == "token_mlp":
        C, Hd, M = 180, 360, case["M"]
        g, b = _ln(C, 2001)
        (w1, b1), (w2, b2) = _lin(Hd, C, 2003), _lin(C, Hd, 2005)
        return dict(x=rnd(M, C, seed=2000 + M, scale=1.5) + 0.3, gamma=g, beta=b, w1=w1, b1=b1, w2=w2, b2=b2)
    if kernel == "token_projmlp":
        C, Hd, M = 180, 360, case["M"]
        g, b = _ln(C, 2101)
        (wp, bp), (w1, b1), (w2, b2) = _lin(C, C, 2103), _lin(Hd, C, 2105), _lin(C, Hd, 2107)
        att = rnd(M, C, seed=2110 + M)
        d = dict(att=att.bfloat16() if case["io"] & 1 else att, x=rnd(M, C, seed=2111 + M, scale=1.5) + 0.3, wp=wp, bp=bp, w1=w1, b1=b1,
                 w2=w2, b2=b2, gamma=g, beta=b)
        if case["c2"]:
            c2 = rnd(M, C, seed=2112 + M)
            d.update(c2=c2.bfloat16() if case["io"] & 2 else c2, c2_scale=rnd(C, seed=2113) * 0.3 + 0.7)
        return d
    if kernel == "token_linear_gated":
        C, Hd, M = 180, 11, case["M"]
        (gw1, gb1), (w, b) = _lin(Hd, C, 2203), _lin(C, C, 2207)
        return dict(x=rnd(M, C, seed=2200 + M, scale=1.5) + 0.3, x2=rnd(M, C, seed=2201 + M), cm=torch.sigmoid(rnd(C, seed=2202)),
                    gw1=gw1, gb1=gb1, gw2=rnd(1, Hd, seed=2205, scale=0.5), gb2=0.13, w=w, b=b, res=rnd(M, C, seed=2209 + M))
    if kernel in ("naf_ffn", "naf_tail"):
        C, M = case["C"], case["M"]
        lg, lb = _ln(C, 2301 + C)
        (w4, b4), (w5, b5) = _lin(2 * C, C, 2303 + C), _lin(C, C, 2305 + C)
        if kernel == "naf_ffn":
            return dict(y=rnd(M, C, seed=2300 + C + M, scale=1.5) + 0.3, w4=w4, b4=b4, w5=w5, b5=b5, ln_g=lg, ln_b=lb,
                        oscale=rnd(C, seed=2307 + C) * 0.3)
        w3, b3 = _lin(C, C, 2309 + C)
        return dict(g=rnd(M, C, seed=2311 + C + M, scale=1.2), x=rnd(M, C, seed=2312 + C + M, scale=1.5) + 0.3, w3=w3, b3=b3, w4=w4, b4=b4,
                    w5=w5, b5=b5, sca=rnd(C, seed=2313 + C) * 0.3 + 1.0, beta=rnd(C, seed=2314 + C) * 0.4, ln_g=lg, ln_b=lb,
                    gamma=rnd(C, seed=2315 + C) * 0.3)
    if kernel == "naf_front":
        C, H, W = case["C"], case["H"], case["W"]
        lg, lb = _ln(C, 2401 + C)
        w1, b1 = _lin(2 * C, C, 2403 + C)
        return dict(x=rnd(1, H, W, C, seed=2400 + C + H, scale=1.5) + 0.3, w1=w1, b1=b1, ln_g=lg, ln_b=lb,
                    wdw=rnd(2 * C, 1, 3, 3, seed=2405 + C, scale=0.3), bdw=rnd(2 * C, seed=2406 + C, scale=0.1))
    if kernel == "sgfn_tail":
        C, c2, H, W = 180, 360, case["H"], case["W"]
        y = torch.nn.functional.gelu(rnd(1, H, W, 2 * c2, seed=2500 + H, scale=1.5) + 0.3)          # what fc1 + GELU hands over
        x2 = y[0, :, :, c2:].reshape(H * W, c2)
        mean = x2.mean(-1)
        stats = torch.stack((mean, 1.0 / torch.sqrt(x2.var(-1, unbiased=False) + 1e-5)), dim=1).contiguous()
        g2, bb2 = _ln(c2, 2501)
        w2, b2 = _lin(C, c2, 2503)
        return dict(y=y, c2=c2, wd=rnd(c2, 1, 3, 3, seed=2505, scale=0.3), bd=rnd(c2, seed=2506, scale=0.1), stats=stats, gamma=g2, beta=bb2,
                    w2=w2, b2=b2, res=rnd(1, H, W, C, seed=2507 + H, scale=1.5) + 0.3 if case["res"] else None)
    raise KeyError(kernel)


REFS = dict(token_mlp=token_mlp_ref, token_projmlp=token_projmlp_ref, token_linear_gated=token_linear_gated_ref, naf_ffn=naf_ffn_ref,
            naf_tail=naf_tail_ref, naf_front=naf_front_ref, sgfn_tail=sgfn_tail_ref)


def reference(kernel: str, case: dict):
    """-> (inputs, StageRef) -- for naf_front (inputs, (gated StageRef, pooled StageRef))."""
    inp = make_inputs(kernel, case)
    return inp, REFS[kernel](**inp)


def gemm_noise_ratio(a, w64, bias) -> float:
    """max |chunked fp32 stand-in - fp64| / (2^-24 (sum |a||w| + |bias|)) for one GEMM stage's operands (as logged in StageRef.gemms)."""
    from lowprec_ref import chunked_fp32_matmul
    y = a.matmul(w64.t())
    mag = a.abs().matmul(w64.abs().t())
    s = chunked_fp32_matmul(a.float(), w64.float())
    if bias is not None:
        y, mag, s = y + bias.double(), mag + bias.double().abs(), s + bias.float()
    return ((s.double() - y).abs() / (U24 * mag.clamp_min(1e-30))).max().item()


def layernorm_fp32(x, gamma, beta, eps):
    """The kernels' two-pass fp32 LayerNorm (ff_common.h ff_frag_ln_stats / ff_frag_ln_step)."""
    x = x.float()
    mean = x.sum(-1, keepdim=True) / x.shape[-1]
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).sum(-1, keepdim=True) / x.shape[-1] + eps)
    return d * rstd * gamma.float() + beta.float()


def ln_noise_ratio(x64, gamma, beta, eps) -> float:
    """max |fp32 LayerNorm - fp64| / (2^-24 max(1, |v|)) on the fp32 image of one LayerNorm's logged operand."""
    xf = x64.float()
    v = layernorm_f64(xf, gamma, beta, eps)
    return ((layernorm_fp32(xf, gamma, beta, eps).double() - v).abs() / (U24 * v.abs().clamp_min(1.0))).max().item()
