"""Stage-rounded fp64 references for the attention kernels of the plain-bf16 ('bf16') contraction mode (pure torch, CPU or GPU):
    window_attn_ref      window_attn_bf16_kernel<1>            csrc/attention_bf16.hip     (ops.window_attn)
    ocab_attn_ref        ocab_attn_kernel<false | true>        csrc/ocab_attn.hip          (ops.ocab_attn, ops.ocab_attn_rows16)
    win_attn_fused_ref   win_attn_fused_v2_kernel<WW, ONES>    csrc/win_attn_fused_v2.inc  (ops.win_attn_fused)
The accounting (round_point, StageRef, compare, assert_caps, the noise constants) is stage_ref's and is imported, not copied.

Inside attention there is ONE hidden rounding point: the un-normalised probability P = exp2(fma(s, log2e, -m log2e)) is cast to bf16
before the PV MFMA.  m is the RUNNING maximum of the online softmax at that moment, so the schedule is part of the arithmetic: each
reference reproduces its kernel's tiles (below) and rounds P relative to the running maximum, in fp64, and nowhere else except at the
casts of values the test controls (q * scale, k, v; in the fused kernel the LayerNorm output and the projected q / k / v).  A tile's
contribution is carried to the end with the exact factor exp(m_tile - m_final), which is what the kernels' `o *= corr` chain multiplies
up to fp32 roundings.
    kernel                      running max per        key order that matters                      denominator                mask
    window_attn_bf16_kernel<1>  128-key chunk (AKC)    window order, chunk c = keys 128c..128c+127, fp32 sum of the UNROUNDED e  += -100
                                                       the ragged last chunk gets -inf
    ocab_attn_kernel            32-key tile            tile T = 3 tr + tc = window rows 4tr..4tr+3, sum of the ROUNDED P         none; zero keys outside
                                                       columns 8tc..8tc+7; 18 tiles, two stages    (V channel 30 = 1)         the image stay in
    win_attn_fused_v2_kernel    32-key tile            tile t = keys 32t..32t+31                   ONES (d == 30): rounded P; ONES: +-7.0625 in q / k
                                                                                                   else the unrounded sum     channels 30 / 31; else -100
(the ballot of the two tile kernels only gates the rescale: m_new = max(m_run, mx) per query either way).

Noise delta at the P rounding point (P = exp(t), t = s - m; everything relative to P, ln2 * log2e = 1):
    noise of s     GEMM_NOISE_C * 2^-24 * (sum |q||k| + |bias|), plus 2^-24 |s| where -100 is added in fp32 (attention_bf16.hip:251,
                   win_attn_fused_v2.inc:339);
    noise of m     the same bound on the running maximum: the largest noise of s over the keys seen so far;
    fma + exp2     counted from attention_bf16.hip:267-279 = ocab_attn.hip:264-269 = win_attn_fused_v2.inc:357-366, in units of 2^-24:
                   |m| (mneg = -m * LOG2E is rounded once at magnitude |m| log2e) + 2 |t| (the fp32 constant LOG2E is within 2^-24 of
                   log2e, and the fma rounds its result t log2e once) + 2 (v_exp_f32 taken as one ulp, as in stage_ref's gelu budget).
    masked ONES    in the shifted border windows of the d == 30 fused kernel the mask rides in q / k channels 30 / 31: same-region scores
                   sit at 2 * 7.0625^2 = 99.76, i.e. in [64, 128) where the fp32 spacing is 2^-17, so the accumulator holding s carries up
                   to half of that, 2^-18, however exact the 30 real channels are.  That term is added to the noise of s (and through it
                   to m's) in those windows only; the two mask products themselves are exact and are NOT put into sum |q||k|.  The
                   |m| term above already covers the rounding of mneg at magnitude 144 (half of 2^-16 there).
Movement.  A fragile P moves the output as move @ |v| / den, and where the denominator sums the rounded P also as |out| sum(move) / den.
A bf16 output (`out_bf16`) is one more rounding point: round_point(out, noise + allow) with noise = (GEMM_NOISE_C + T + 3) 2^-24
sum(P |v|) / den (the PV accumulation; T rescales, the reciprocal as one ulp and the product) -- its movement is then the allowance.
The q * scale cast of the stand-alone kernels (attention_bf16.hip:84-96, ocab_attn.hip:195) has NO movement: it is one IEEE fp32
multiply of two exact inputs, which the reference repeats bit for bit (torch fp32 multiply), like naf_tail's g * sca in stage_ref.

The fused kernel gets FIXED-POINT inputs (make_inputs): every stage ahead of the exponent is then exact in fp32 whatever the summation
order, which the reference asserts from itself alone (the LayerNorm rounding point has zero movement under ln_noise; every partial sum
of the projections and of S, the +99.76 of masked ONES windows and the -100 of the d == 32 form included, is below 2^24 grid steps),
and P is the only fragile rounding point.  The grids are coarser than a first guess of 2^-6 weights: with x on 2^-1, gamma in
{0.5, 1, 2}, beta on 2^-2 the operand is on 2^-2; weights on 2^-5 and scale 0.25 put q on 2^-9 and k on 2^-7, S on 2^-16, so the bound is
256 and holds the 99.76.  Weights are kept to |w| <= 2/32 so that the logits stay of order one.  v_out must then equal the fp64 value bit
for bit, the bf16 xn side output the rounded operand, the fp32 one within 2e-6.  Generic-input coverage of the fused kernel (a flip
model through LayerNorm, projection and softmax is not part of this module) stays in tests/test_ops_gpu.py
(test_win_attn_fused_hat / _dat_branches).  pack_win_attn accepts d = 32, K = 192 (6 heads), so the non-ONES instantiation has a case.

The stand-alone kernels get q / k ~ randn and v ~ randn + 0.75 (a non-zero mean output, so that a wrong denominator shows), scale
d ** -0.5, once flat (near-uniform softmax) and once sharpened (q * 4: mean top probability about 0.5).

tests/test_attn_ref_cpu.py checks this module against fp32 stand-ins and mutants of them on the CPU; tests/test_lowprec_attn_gpu.py
holds the kernels to it."""
import functools
import math
from collections import namedtuple

import torch

from lowprec_ref import FP32_CHAIN_TOL, bf16_rne, layernorm_f64, operand_w  # noqa: F401  (FP32_CHAIN_TOL re-exported)
from stage_ref import GEMM_NOISE_C, U24, StageRef, allowance_shares, assert_caps, case_name, compare, ln_noise, rnd, round_point  # noqa: F401

MASK_Q = 7.0625              # win_attn_fused_v2.inc:120: the shift mask's q / k channel value (bf16-exact; 2 * 7.0625^2 = 99.7578125)
NEG = -100.0                 # the reference implementations' mask value

# A softmax problem in the kernel's own terms.  q [G, 256, dk], k [G, Nk, dk], v [G, Nk, d]: fp64 tensors holding the bf16 operands, keys
# in the kernel's tile order, Nk a multiple of `tile`; bias [G, 256, Nk] fp64 (the fp32 table values); neg [G, 256, Nk] 0 or -100, added
# after the accumulation; live [G, 1 or 256, Nk] False = the key is not there (-inf: the ragged tail); smask [G, 256, Nk] or None: exact
# mask-channel products (ONES) added INSIDE the accumulation; s_extra [G, 1, 1]: extra noise of s; G = windows x heads, window-major.
# qtok [windows, 256]: token of every query or -1.
Problem = namedtuple("Problem", "q k v bias neg live smask s_extra tile den_rounded qtok heads d ntok out_bf16")


# ---------------------------------------------------------------------------------------------------------------------
# window geometry (attention_bf16.hip:53-73, :110-128; ocab_attn.hip:59-64, :75-79; win_attn_fused_v2.inc:86-99)
def geometry(H, W, Hp, Wp, wh, ww, kh, kw, sh, sw, use_mask):
    nwy, nwx = Hp // wh, Wp // ww
    wy = torch.arange(nwy).repeat_interleave(nwx)[:, None]          # block index = (wy * nwx + wx) (* heads + head)
    wx = torch.arange(nwx).repeat(nwy)[:, None]

    def region(y, x):
        ry = torch.where(y < Hp - wh, 0, torch.where(y < Hp - sh, 1, 2))
        rx = torch.where(x < Wp - ww, 0, torch.where(x < Wp - sw, 1, 2))
        return 3 * ry + rx

    qi = torch.arange(wh * ww)[None, :]
    qyl, qxl = qi // ww, qi % ww
    qy, qx = wy * wh + qyl, wx * ww + qxl
    oy, ox = (qy + sh) % Hp, (qx + sw) % Wp
    qtok = torch.where((oy < H) & (ox < W), oy * W + ox, -1)
    ki = torch.arange(kh * kw)[None, :]
    kyl, kxl = ki // kw, ki % kw
    ky, kx = wy * wh - (kh - wh) // 2 + kyl, wx * ww - (kw - ww) // 2 + kxl
    inb = (ky >= 0) & (kx >= 0) & (ky < Hp) & (kx < Wp)
    yy, xx = (ky + sh) % Hp, (kx + sw) % Wp
    ktok = torch.where(inb & (yy < H) & (xx < W), yy * W + xx, -1)
    zero = torch.zeros_like(qtok)
    qreg = region(qy, qx) if use_mask else zero
    kreg = torch.where(inb, region(ky, kx), 0) if use_mask else torch.zeros_like(ktok)
    blk = ((wy == nwy - 1) | (wx == nwx - 1)).reshape(-1) & bool(use_mask)
    return dict(qtok=qtok, ktok=ktok, qreg=qreg, kreg=kreg, blk=blk, qyl=qyl[0], qxl=qxl[0], kyl=kyl[0], kxl=kxl[0], nwin=nwy * nwx)


def gather_bias(rel, wh, ww, kh, kw, geo, mut=None):
    """rel [heads, n] -> bias [heads, 256, nk] (window key order).  Keys == query window: n = (2wh-1)(2ww-1), index
    (qy - ky + wh-1)(2ww-1) + (qx - kx + ww-1) (attention_bf16.hip:178).  Overlapping keys: n = (wh+kh-1)^2, index
    ((ky - qy + a)(wh+kh-1) + (kx - qx + a)) mod n, a = wh - kh + 1 (attention_bf16.hip:160; the reference's wrapped negative indices).
    mut: 'swap' = q and k exchanged in the gather, 'off' = one table entry further for query row 5 (the CPU test's mutants)."""
    dy = geo["qyl"][:, None] - geo["kyl"][None, :]
    dx = geo["qxl"][:, None] - geo["kxl"][None, :]
    if mut == "swap":
        dy, dx = -dy, -dx
    n = rel.shape[1]
    if (kh, kw) == (wh, ww):
        idx = (dy + wh - 1) * (2 * ww - 1) + (dx + ww - 1)
    else:
        a = wh - kh + 1
        idx = ((-dy + a) * (ww + kw - 1) + (-dx + a)) % n
    if mut == "off":
        idx = idx.clone()
        idx[5] = (idx[5] + 1) % n
    return rel[:, idx]


def _rows(t, tok, off, heads, d):
    """t [ntok + 1, ch] (last row = the zero / pad token), tok [nwin, n] with -1 = pad -> [nwin, heads, n, d]."""
    g = t[tok][..., off:off + heads * d]
    return g.reshape(tok.shape[0], tok.shape[1], heads, d).permute(0, 2, 1, 3)


def _pad_keys(x, nkp, value=0.0):
    """Pad the key axis of k / v [..., keys, channels] up to nkp."""
    return x if x.shape[-2] == nkp else torch.cat([x, x.new_full(x.shape[:-2] + (nkp - x.shape[-2], x.shape[-1]), value)], dim=-2)


def _pad_last(x, nkp, value):
    """Pad the key axis of a score-shaped tensor [..., keys] up to nkp."""
    return x if x.shape[-1] == nkp else torch.cat([x, x.new_full(x.shape[:-1] + (nkp - x.shape[-1],), value)], dim=-1)


def _finish(q, k, v, bias, neg, live, smask, s_extra, tile, den_rounded, geo, heads, d, ntok, out_bf16):
    G = q.shape[0] * q.shape[1]
    f = lambda x: None if x is None else x.reshape((G,) + tuple(x.shape[2:]))          # noqa: E731
    return Problem(f(q), f(k), f(v), f(bias), f(neg), f(live), f(smask), f(s_extra), tile, den_rounded, geo["qtok"], heads, d, ntok, out_bf16)


def window_problem(qkv, rel, H, W, Hp, Wp, win, kwin, shift, use_mask, heads, d, scale, q_off, k_off, v_off, bias_mut=None, mask_mut=None,
                   chan_mut=0, **_):
    """ops.window_attn in plain bf16 (window_attn_bf16_kernel<1>)."""
    (wh, ww), (kh, kw) = win, kwin
    geo = geometry(H, W, Hp, Wp, wh, ww, kh, kw, shift[0], shift[1], use_mask)
    rows = torch.cat([qkv.reshape(H * W, -1).float(), torch.zeros(1, qkv.shape[-1])])
    sc = torch.tensor(scale, dtype=torch.float32)
    q = bf16_rne(_rows(rows, geo["qtok"], q_off + chan_mut, heads, d) * sc).double()      # attention_bf16.hip:84-96: (__bf16)(q * scale), one IEEE multiply
    k = bf16_rne(_rows(rows, geo["ktok"], k_off, heads, d)).double()                      # attention_bf16.hip:218: k_h = (__bf16)kv[i]
    v = bf16_rne(_rows(rows, geo["ktok"], v_off, heads, d)).double()                      # attention_bf16.hip:218: v_h = (__bf16)vv[i]
    nk = kh * kw
    nkp = (nk + 127) // 128 * 128
    nwin = geo["nwin"]
    bias = gather_bias(rel.double(), wh, ww, kh, kw, geo, bias_mut)[None].expand(nwin, heads, 256, nk)
    differ = (geo["qreg"][:, :, None] != geo["kreg"][:, None, :])[:, None]               # attention_bf16.hip:251
    neg = torch.where(differ, NEG if mask_mut != "omit" else 0.0, 0.0).double().expand(nwin, heads, 256, nk)
    live = _pad_last(torch.ones(nwin, heads, 1, nk, dtype=torch.bool), nkp, False)        # attention_bf16.hip:258: the ragged tail = -inf
    return _finish(q, _pad_keys(k, nkp), _pad_keys(v, nkp), _pad_last(bias, nkp, 0.0), _pad_last(neg, nkp, 0.0), live, None, None, 128, False,
                   geo, heads, d, H * W, False)


def ocab_tile_order():
    """Position in the 24 x 24 key window of key 32 T + kappa of ocab_attn_kernel (ocab_attn.hip:59-62)."""
    i = torch.arange(576)
    T, kap = i // 32, i % 32
    return (4 * (T // 3) + kap // 8) * 24 + 8 * (T % 3) + kap % 8


def ocab_problem(qkv, rel, H, W, heads, d, scale, q_off, k_off, v_off, out_bf16=False, bias_mut=None, pad_mut=None, chan_mut=0, **_):
    """ops.ocab_attn / ops.ocab_attn_rows16 (ocab_attn_kernel): the rows form reads the same operands, already rounded."""
    geo = geometry(H, W, H, W, 16, 16, 24, 24, 0, 0, False)
    rows = torch.cat([qkv.reshape(H * W, -1).float(), torch.zeros(1, qkv.shape[-1])])
    sc = torch.tensor(scale, dtype=torch.float32)
    order = ocab_tile_order()
    ktok = geo["ktok"][:, order]
    q = bf16_rne(_rows(rows, geo["qtok"], q_off + chan_mut, heads, d) * sc).double()      # ocab_attn.hip:195-196: (__bf16)(q * scale)
    k = bf16_rne(_rows(rows, ktok, k_off, heads, d)).double()                             # ocab_attn.hip:151: (__bf16)(ok ? k : 0)
    v = bf16_rne(_rows(rows, ktok, v_off, heads, d)).double()                             # ocab_attn.hip:151: (__bf16)(ok ? v : 0)
    nwin = geo["nwin"]
    bias = gather_bias(rel.double(), 16, 16, 24, 24, geo, bias_mut)[:, :, order][None].expand(nwin, heads, 256, 576)
    neg = torch.zeros(1, 1, 1, 1, dtype=torch.float64).expand(nwin, heads, 256, 576)
    live = torch.ones(nwin, heads, 1, 576, dtype=torch.bool)
    if pad_mut == "remove":                              # the CPU test's mutant: zero keys outside the image taken out of the softmax
        live = (ktok >= 0)[:, None, None, :].expand(nwin, heads, 1, 576)
    return _finish(q, k, v, bias, neg, live, None, None, 32, True, geo, heads, d, H * W, out_bf16)


def _multiple(t, step):
    return bool((t / step == (t / step).round()).all())


def fused_problem(x, gamma, beta, wqkv, bqkv, rel, H, W, Hp, Wp, win, shift, use_mask, heads, d, scale, head0=0, nheads=None, zero_pad=False,
                  out_bf16=False, eps=1e-5, bias_mut=None, mask_mut=None, chan_mut=0, **_):
    """ops.win_attn_fused in plain bf16 (win_attn_fused_v2_kernel<WW, d == 30>) on fixed-point inputs
    -> (Problem, side outputs dict(xn, xn_bf16, v), the exactness facts).  wqkv [3 C, K] rows q | k | v, head-major; rel [heads, n]."""
    wh, ww = win
    nheads = heads - head0 if nheads is None else nheads
    ones = d == 30
    C, K = heads * d, x.shape[-1]
    geo = geometry(H, W, Hp, Wp, wh, ww, wh, ww, shift[0], shift[1], use_mask)
    xr = torch.cat([x.reshape(H * W, K).double(), torch.zeros(1, K, dtype=torch.float64)])      # the pad token: x = 0 (win_attn_fused_v2.inc:138)
    vln = layernorm_f64(xr, gamma, beta, eps)
    vln[-1] = beta.double()                                                                    # LayerNorm of the zero row: (0 - 0) * rstd * g + b, exact
    xn, mv_ln = round_point(vln, ln_noise(vln))                                                # win_attn_fused_v2.inc:191: xh = (__bf16)f
    mv_ln = mv_ln[:-1]                                                                         # (the pad row carries no noise)
    facts = dict(ln_move=mv_ln.max().item())
    gx, gw = 2.0 ** -2, 2.0 ** -5
    assert _multiple(xn, gx), "the LayerNorm operand is not on its grid"
    sc = torch.tensor([scale] * C + [1.0] * (2 * C), dtype=torch.float32)[:, None]
    w64 = operand_w(wqkv.float() * sc)                                                         # prep.pack_win_attn: scale folded into q, hi plane
    b64 = (bqkv.float() * sc[:, 0]).double()
    assert _multiple(w64[C:], gw) and _multiple(w64[:C], gw * scale) and _multiple(b64, gx * gw * scale) and _multiple(rel.double(), 2.0 ** -4)
    proj = xn.matmul(w64.t()) + b64                                                            # win_attn_fused_v2.inc:241-242 (bias = C-in of the MFMAs)
    mag = xn.abs().matmul(w64.abs().t()) + b64.abs()
    facts["proj_q"] = mag[:, :C].max().item() / (2.0 ** 24 * gx * gw * scale)                    # < 1: every partial sum of q is exact in fp32
    facts["proj_kv"] = mag[:, C:].max().item() / (2.0 ** 24 * gx * gw)
    v_side = proj[:-1, 2 * C:].clone()                                                         # win_attn_fused_v2.inc:297: vout = the fp32 accumulator
    cast = bf16_rne(proj.float()).double()                                                     # win_attn_fused_v2.inc:247, :268, :290: (__bf16)acc
    if zero_pad:                                                                               # win_attn_fused_v2.inc:257-261, :280-284
        cast[-1, C:] = 0.0
    sl = slice(head0 * d, (head0 + nheads) * d)
    q = _rows(cast[:, :C].roll(-chan_mut, 1)[:, sl], geo["qtok"], 0, nheads, d)
    k = _rows(cast[:, C:2 * C][:, sl], geo["ktok"], 0, nheads, d)
    v = _rows(cast[:, 2 * C:][:, sl], geo["ktok"], 0, nheads, d)
    nwin = geo["nwin"]
    bias = gather_bias(rel.double()[head0:head0 + nheads], wh, ww, wh, ww, geo, bias_mut)[None].expand(nwin, nheads, 256, 256)
    differ = (geo["qreg"][:, :, None] != geo["kreg"][:, None, :])[:, None]
    smask, s_extra = None, None
    neg = torch.zeros(1, 1, 1, 1, dtype=torch.float64).expand(nwin, nheads, 256, 256)
    if ones and use_mask and mask_mut != "omit":
        # win_attn_fused_v2.inc:120, :243, :262: q / k channels 30 / 31 = +-7.0625 by row / column region 2, in the border windows only
        blk = geo["blk"][:, None].double()
        cy = torch.where(geo["qreg"] // 3 == 2, -MASK_Q, MASK_Q) * blk
        cx = torch.where(geo["qreg"] % 3 == 2, -MASK_Q, MASK_Q) * blk
        smask = (cy[:, :, None] * cy[:, None, :] + cx[:, :, None] * cx[:, None, :])[:, None].expand(nwin, nheads, 256, 256)
        s_extra = (blk * 2.0 ** -18).reshape(nwin, 1, 1, 1).expand(nwin, nheads, 1, 1)
    elif use_mask and mask_mut != "omit":
        neg = torch.where(differ, NEG, 0.0).double().expand(nwin, nheads, 256, 256)             # win_attn_fused_v2.inc:339
    smag = q.abs().matmul(k.abs().transpose(-1, -2)) + bias.abs() + (0.0 if smask is None else smask.abs()) + neg.abs()
    facts["scores"] = smag.max().item() / (2.0 ** 24 * (gx * gw * scale) * (gx * gw))            # < 1: every partial sum of S is exact in fp32
    live = torch.ones(nwin, nheads, 1, 256, dtype=torch.bool)
    pb = _finish(q, k, v, bias, neg, live, smask, s_extra, 32, ones, geo, nheads, d, H * W, out_bf16)
    return pb, dict(xn=vln[:-1], xn_bf16=xn[:-1], v=v_side[:, sl]), facts


def assert_exact(facts, name):
    """The fused cases' exactness facts, from the reference alone."""
    print(f"ATTN_REF_EXACT {name}: LayerNorm movement {facts['ln_move']:.1e}; largest partial sum / (2^24 grid steps): q {facts['proj_q']:.3f}, "
          f"k / v {facts['proj_kv']:.3f}, S {facts['scores']:.3f}")
    assert facts["ln_move"] == 0.0, (name, facts)
    assert facts["proj_q"] < 1.0 and facts["proj_kv"] < 1.0 and facts["scores"] < 1.0, (name, facts)


# ---------------------------------------------------------------------------------------------------------------------
# the reference proper
def solve(pb: Problem):
    """-> (StageRef over the image's tokens [1, ntok, heads * d], info dict(fragile = share of live P that are fragile))."""
    G, Q, Nk = pb.bias.shape
    T = Nk // pb.tile
    kt = pb.k.transpose(1, 2)
    s = pb.q.matmul(kt) + pb.bias
    mag = pb.q.abs().matmul(pb.k.abs().transpose(1, 2)) + pb.bias.abs()
    if pb.smask is not None:
        s = s + pb.smask
    ns = GEMM_NOISE_C * U24 * mag
    if pb.s_extra is not None:
        ns = ns + pb.s_extra
    masked = pb.neg != 0
    s = s + pb.neg
    ns = ns + torch.where(masked, U24 * s.abs(), 0.0)
    live = pb.live.expand(G, Q, Nk)
    ninf = torch.full((), -math.inf, dtype=torch.float64)
    s = torch.where(live, s, ninf)
    ns = torch.where(live, ns, 0.0)
    m_run = s.reshape(G, Q, T, pb.tile).amax(-1).cummax(-1).values                             # the running maximum after every tile
    assert torch.isfinite(m_run).all(), "a first tile without a key"
    nm = ns.reshape(G, Q, T, pb.tile).amax(-1).cummax(-1).values.repeat_interleave(pb.tile, -1)
    m = m_run.repeat_interleave(pb.tile, -1)
    t = torch.where(live, s - m, 0.0)
    e = torch.where(live, torch.exp(t), 0.0)
    delta = e * (ns + nm + U24 * (m.abs() + 2.0 * t.abs() + 2.0))
    P, mv = round_point(e, delta)             # attention_bf16.hip:281 / ocab_attn.hip:269 / win_attn_fused_v2.inc:366: (__bf16)exp2(fma(s, LOG2E, mneg))
    w = torch.exp(m - m_run[..., -1:])
    Pw, mw = P * w, mv * w
    num = Pw.matmul(pb.v)
    den = (Pw if pb.den_rounded else e * w).sum(-1, keepdim=True)
    out = num / den
    allow = mw.matmul(pb.v.abs()) / den
    if pb.den_rounded:
        allow = allow + out.abs() * mw.sum(-1, keepdim=True) / den
    if pb.out_bf16:                           # ocab_attn.hip:285-286 / win_attn_fused_v2.inc:394-395: (__bf16)(o * inv)
        noise = (GEMM_NOISE_C + T + 3) * U24 * Pw.matmul(pb.v.abs()) / den
        out, allow = round_point(out, noise + allow)
    fragile = ((mv > 0) & live).double().sum().item() / live.double().sum().item()
    # scatter [windows, heads, 256, d] to the image's token rows
    nwin = pb.qtok.shape[0]
    hd = pb.heads * pb.d
    o = out.reshape(nwin, pb.heads, Q, pb.d).permute(0, 2, 1, 3).reshape(nwin * Q, hd)
    a = allow.reshape(nwin, pb.heads, Q, pb.d).permute(0, 2, 1, 3).reshape(nwin * Q, hd)
    tok = pb.qtok.reshape(-1)
    ok = tok >= 0
    assert int(ok.sum()) == pb.ntok and torch.equal(tok[ok].sort().values, torch.arange(pb.ntok)), "every token is the query of exactly one window"
    ref = torch.zeros(pb.ntok, hd, dtype=torch.float64)
    alw = torch.zeros(pb.ntok, hd, dtype=torch.float64)
    ref[tok[ok]], alw[tok[ok]] = o[ok], a[ok]
    sr = StageRef(ref.reshape(1, pb.ntok, hd), alw.reshape(1, pb.ntok, hd), (1, pb.ntok, hd), None, [], [])
    return sr, dict(fragile=fragile)


def window_attn_ref(**inp):
    return solve(window_problem(**inp))


def ocab_attn_ref(**inp):
    return solve(ocab_problem(**inp))


def win_attn_fused_ref(**inp):
    """-> (StageRef, info) with info carrying the side outputs' references and the exactness facts."""
    pb, side, facts = fused_problem(**inp)
    sr, info = solve(pb)
    info.update(side=side, facts=facts)
    return sr, info


# ---------------------------------------------------------------------------------------------------------------------
# cases and inputs (seeded CPU generators; CPU tensors, the GPU test moves them)
HEADS, D = 6, 30
CASES = {
    "window_attn": [
        # HAT 16x16: one window holding every mask region, flat and sharpened; six windows without a shift
        dict(kind="hat", H=16, W=16, shift=8, sharp=False, odd=False),
        dict(kind="hat", H=16, W=16, shift=8, sharp=True, odd=False),
        dict(kind="hat", H=32, W=48, shift=0, sharp=True, odd=False),
        # OCAB keys 24x24 on 32x32: 576 keys = 4.5 chunks, every window touches a border (zero keys)
        dict(kind="ocab", H=32, W=32, shift=0, sharp=False, odd=False),
        # DAT 8x32 / 32x8 on 40x72 (Hp, Wp = 64, 96), shifted and masked, channel halves with o_off
        dict(kind="dat0", H=40, W=72, shift=1, sharp=True, odd=False),
        dict(kind="dat1", H=40, W=72, shift=1, sharp=False, odd=False),
        # odd q_off / o_off: the scalar vec_q == 0 and vec_out == 0 paths
        dict(kind="hat", H=16, W=16, shift=8, sharp=False, odd=True),
    ],
    "ocab_attn": [
        dict(H=32, W=32, rows16=False, out_bf16=False, ld=False, sharp=False),
        dict(H=32, W=32, rows16=True, out_bf16=False, ld=False, sharp=True),
        dict(H=32, W=32, rows16=False, out_bf16=True, ld=False, sharp=False),
        dict(H=16, W=48, rows16=False, out_bf16=False, ld=True, sharp=True),
        dict(H=16, W=48, rows16=True, out_bf16=True, ld=True, sharp=False),
    ],
    "win_attn_fused": [
        dict(kind="hat", H=16, W=16, shift=8, d=30, xn=None, out_bf16=False),
        dict(kind="hat", H=32, W=48, shift=0, d=30, xn="f32", out_bf16=False),
        dict(kind="hat", H=32, W=48, shift=0, d=30, xn="bf16", out_bf16=True),
        dict(kind="dat0", H=40, W=72, shift=1, d=30, xn=None, out_bf16=False),
        dict(kind="dat1", H=40, W=72, shift=1, d=30, xn=None, out_bf16=False),
        dict(kind="hat", H=32, W=32, shift=8, d=32, xn=None, out_bf16=False),          # the non-ONES instantiation (K = 192)
    ],
}


def _ints(*shape, lo, hi, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _fixed_rows(n, K, seed):
    """Signed permutations of a multiset with mean 0 and mean square exactly 1: K = 180: 50 x 0.5, 100 x 1.0, 30 x 1.5;
    K = 192: 60 x 0.5, 96 x 1.0, 36 x 1.5; each class half positive."""
    cnt = {180: (50, 100, 30), 192: (60, 96, 36)}[K]
    base = torch.cat([torch.full((c // 2,), s * val) for c, val in zip(cnt, (0.5, 1.0, 1.5)) for s in (1.0, -1.0)])
    assert base.numel() == K and base.sum().item() == 0.0 and base.pow(2).sum().item() == float(K)
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.stack([base[torch.randperm(K, generator=g)] for _ in range(n)])


def _win_geometry(kind, H, W, shift):
    if kind == "hat":
        return dict(Hp=H, Wp=W, win=(16, 16), kwin=(16, 16), shift=(shift, shift), use_mask=shift > 0, heads=HEADS, hsel=(0, HEADS))
    if kind == "ocab":
        return dict(Hp=H, Wp=W, win=(16, 16), kwin=(24, 24), shift=(0, 0), use_mask=False, heads=HEADS, hsel=(0, HEADS))
    wh, ww = (8, 32) if kind == "dat0" else (32, 8)
    Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
    return dict(Hp=Hp, Wp=Wp, win=(wh, ww), kwin=(wh, ww), shift=(wh // 2, ww // 2) if shift else (0, 0), use_mask=bool(shift), heads=3,
                hsel=(0, 3) if kind == "dat0" else (3, 3))


def make_inputs(kernel: str, case: dict) -> dict:
    """The reference's keyword arguments for one case (what the kernel's entry point needs is derived from them by the tests)."""
    H, W = case["H"], case["W"]
    C = HEADS * D
    if kernel == "window_attn":
        geo = _win_geometry(case["kind"], H, W, case["shift"])
        (wh, ww), (kh, kw) = geo["win"], geo["kwin"]
        heads = geo["heads"]
        base = geo["hsel"][0] * D + (1 if case["odd"] else 0)            # DAT: the branch's channel half; odd: every slice one float in
        width = 3 * C + (2 if case["odd"] else 0)
        seed = 3000 + 7 * H + W + (50 if case["sharp"] else 0) + len(case["kind"])
        qkv = rnd(1, H, W, width, seed=seed)
        qs = slice(base, base + heads * D)
        if case["sharp"]:
            qkv[..., qs] *= 4.0
        qkv[..., 2 * C + base:2 * C + base + heads * D] += 0.75
        n = (2 * wh - 1) * (2 * ww - 1) if (kh, kw) == (wh, ww) else (wh + kh - 1) ** 2
        return dict(qkv=qkv, rel=rnd(heads, n, seed=seed + 1, scale=0.5), H=H, W=W, Hp=geo["Hp"], Wp=geo["Wp"], win=geo["win"], kwin=geo["kwin"],
                    shift=geo["shift"], use_mask=geo["use_mask"], heads=heads, d=D, scale=D ** -0.5, q_off=base, k_off=C + base,
                    v_off=2 * C + base, o_off=base)
    if kernel == "ocab_attn":
        seed = 3100 + 7 * H + W + (50 if case["sharp"] else 0)
        qkv = rnd(1, H, W, 3 * C, seed=seed)
        if case["sharp"]:
            qkv[..., :C] *= 4.0
        qkv[..., 2 * C:] += 0.75
        return dict(qkv=qkv, rel=rnd(HEADS, 39 * 39, seed=seed + 1, scale=0.5), H=H, W=W, heads=HEADS, d=D, scale=D ** -0.5, q_off=0, k_off=C,
                    v_off=2 * C, out_bf16=case["out_bf16"])
    if kernel == "win_attn_fused":
        d = case["d"]
        C = HEADS * d
        geo = _win_geometry(case["kind"], H, W, case["shift"])
        wh, ww = geo["win"]
        seed = 3200 + 7 * H + W + d + len(case["kind"])
        # beta: multiples of 0.25 that cannot cancel x * gamma (|x gamma| is one of 0.25 .. 3 in steps that miss these): a zero operand
        # would sit between two tiny bf16 values and be fragile for no reason
        betas = torch.tensor([0.0, 1.25, -1.25, 1.75, -1.75, 2.5, -2.5])
        return dict(x=_fixed_rows(H * W, C, seed).reshape(1, H, W, C), gamma=torch.tensor([0.5, 1.0, 2.0])[_ints(C, lo=0, hi=2, seed=seed + 1).long()],
                    beta=betas[_ints(C, lo=0, hi=6, seed=seed + 2).long()], wqkv=_ints(3 * C, C, lo=-2, hi=2, seed=seed + 3) / 32.0,
                    bqkv=_ints(3 * C, lo=-8, hi=8, seed=seed + 4) / 16.0, rel=_ints(HEADS, (2 * wh - 1) * (2 * ww - 1), lo=-16, hi=16, seed=seed + 5) / 16.0,
                    H=H, W=W, Hp=geo["Hp"], Wp=geo["Wp"], win=geo["win"], shift=geo["shift"], use_mask=geo["use_mask"], heads=HEADS, d=d, scale=0.25,
                    head0=geo["hsel"][0], nheads=geo["hsel"][1], zero_pad=case["kind"] != "hat", out_bf16=case["out_bf16"])
    raise KeyError(kernel)


PROBLEMS = dict(window_attn=window_problem, ocab_attn=ocab_problem, win_attn_fused=lambda **k: fused_problem(**k)[0])
REFS = dict(window_attn=window_attn_ref, ocab_attn=ocab_attn_ref, win_attn_fused=win_attn_fused_ref)


@functools.lru_cache(maxsize=None)
def _reference(kernel, key):
    inp = make_inputs(kernel, dict(key))
    sr, info = REFS[kernel](**inp)
    return inp, sr, info


def reference(kernel: str, case: dict):
    """-> (inputs, StageRef, info), computed once per case and shared (callers leave them unchanged)."""
    return _reference(kernel, tuple(sorted(case.items())))


def expand_biasT(inp):
    """window_attn's expanded table [heads, nk, 256] (window key order) from the compact one: what ops.window_attn takes as biasT."""
    (wh, ww), (kh, kw) = inp["win"], inp["kwin"]
    geo = geometry(inp["H"], inp["W"], inp["Hp"], inp["Wp"], wh, ww, kh, kw, inp["shift"][0], inp["shift"][1], inp["use_mask"])
    return gather_bias(inp["rel"], wh, ww, kh, kw, geo).transpose(1, 2).contiguous()


def ocab_rows16(qkv, scale):
    """The head-padded bf16 rows ops.ocab_attn_rows16 reads, from the same values, as ops.token_linear_rows16 writes them from
    prep.pack_ocab_qkv's weights: head h of q / k / v at column 192 j + 32 h, 30 channels and two exact zeros, q multiplied by the scale
    in fp32 before the rounding."""
    B, H, W, _ = qkv.shape
    C = HEADS * D
    s = torch.ones(3, 1, 1, dtype=torch.float32)
    s[0] = torch.tensor(scale, dtype=torch.float32)
    rows = torch.zeros(B, H, W, 3, HEADS, 32, dtype=torch.bfloat16)
    rows[..., :D] = (qkv.reshape(B, H, W, 3, HEADS, D).float() * s).bfloat16()
    return rows.reshape(B, H, W, 3 * HEADS * 32)
