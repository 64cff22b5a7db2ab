"""fp64 references and per-element error bounds for DAT's channel attention (pure torch / numpy, no GPU):
    chan_qkv_blocks_ref    chan_qkv_kernel<1 | 3>                               csrc/chan_qkv.hip    (ff_chan_qkv)
    chan_gram_blocks_ref   chan_gram_kernel                                     csrc/fusion_ops.hip  (stage 1 of ff_chan_attn_weights)
    chan_finish_ref        chan_reduce_body + chan_attn_weights_body            csrc/fusion_ops.hip  (ff_chan_attn_finish / _images, stages 2, 3
                                                                                                       of ff_chan_attn_weights)
What is compared is not the softmaxed 180 x 180 matrix alone but every PARTIAL BLOCK the first kernel leaves in `work`: nblk blocks of
5760 floats, [6][30][30] grams G_h[i][j] = sum_t q[t][30 h + i] k[t][30 h + j], then 180 sums of q^2, then 180 sums of k^2, one block per
workgroup.  A mistake confined to one workgroup, one wave or one token is then held against that block's own magnitude instead of
being diluted by 1 / nblk and a softmax.

Every reference returns `ref` and `mag` (fp64, per element) and, for generic inputs, `extra` (fp64, per element, absolute).  The
assertion is per element, never per tensor maximum (check()):

    |kernel - ref| <= C * 2^-24 * mag + extra ;        an element with mag == 0 and extra == 0 must be exactly 0.

mag is the sum of the absolute values of the terms of the element: sum_t |q^||k^| for a gram entry (q^, k^ the operands the MFMA sees),
sum_t q^2 for a norm, sum_b |partial| for the reduction over blocks.

Constants of the reductions.  None was fitted to a kernel's output.  C_GRAM_MEASURED, C_NORM_MEASURED and C_REDUCE_MEASURED are MEASURED on the CPU by
tests/test_chan_ref_cpu.py: a stand-in plays the kernel's arithmetic with a strictly sequential fp32 accumulation of the same fp32
products in token (block) order, and the largest |stand-in - ref| / (2^-24 mag) over the case tables below is recorded.  The kernels,
which split the same sums over MFMA steps, waves and slices, are held to REDUCTION_FACTOR = 4 times that (stage_ref.GEMM_NOISE_FACTOR,
train_ref.REDUCTION_FACTOR).  The CPU test repeats the measurement and asserts that it stays within 1.25 * MEASURED.

ff_chan_qkv, stage by stage (csrc/chan_qkv.hip):
    :78-104   f = (x - mean) * rstd * gamma + beta, two-pass fp32 LayerNorm over the K = 180 channels
    :105-107  xh = (__bf16)f, xl = (__bf16)(f - xh)                       nterms == 1 uses xh alone
    :128-140  acc = bias + xh wh (+ xl wh + xh wl for nterms == 3; lo * lo is dropped), wh / wl the planes of prep.pack_chan_qkv
    :165      tokens >= M are zeroed AFTER the bias
    :166      norm += f * f on the UNROUNDED accumulator
    :167-169  qh = (__bf16)f, ql = (__bf16)(f - qh)
    :186-191  G += qh kh (+ qh kl + ql kh for nterms == 3; lo * lo dropped), 16 tokens per MFMA step, two steps per wave
    :199-212  the eight waves' tiles and norms summed in wave order, written in ff_chan_attn_finish's layout
    :217-240  v = the fp32 accumulator, rows < M, columns < 180
Two input families.
  EXACT.  x = attn_ref._fixed_rows (mean 0, mean square exactly 1), gamma in {0.5, 1, 2}, beta on 2^-2, weights on 2^-5 with |w| <= 2/32,
    bias on 2^-4, and eps = 0, so that rstd is exactly 1: f lies on the 2^-2 grid, (__bf16)f is exact and its lo part is exactly 0 (with
    eps = 1e-5 the lo part would be fp32 noise).  q, k, v lie on 2^-7 and every partial sum is below 2^24 grid steps, so they are exact
    fp32 numbers whatever the order -- asserted from the reference alone (assert_exact).  v must then be BIT-EQUAL in both modes, (__bf16)q is
    a deterministic rounding the reference repeats, and only the fp32 summation order of grams and norms remains: extra = 0, no flip
    accounting, no allowance caps.
  CORRELATED.  x generic; wk = per head a signed permutation of wq's rows * 0.8 + 0.6 * noise, so that k channel i follows q channel
    pi(i) with cosine up to about 0.8 and, at temperatures 0.5 .. 8, the softmax rows are peaked.  (i.i.d. q and k keep the cosines within
    +-0.3 and every weight in [0.026, 0.046]: a missing temperature or a transposed gram moves such a matrix by 1e-2 at most.)  The last
    32 tokens are built from three rows of wq each (and carry 4 x the amplitude, which the LayerNorm removes again): their q and k are
    several times the typical size, so the tail wave is not lost in its block's sum.  `extra` is a forward bound with counted roundings,
    computed from the reference alone.  With u = 2^-9 (plain bf16) and S = 2^-16 (split bf16), N_LN = stage_ref.ln_noise and
    N_G = stage_ref.GEMM_NOISE_C 2^-24:
      nterms == 1   the reference repeats every rounding, so kernel and reference part only where fp32 noise flips one; the budget
                    nevertheless charges EVERY operand element u of its magnitude -- xn, w, q^ and k^, 2^-9 each -- which covers a
                    flip (one element moving by at most 2^-7 of itself) as long as flips carry under a quarter of a sum's weight;
                    fp32 noise of a few 2^-24 against a bf16 spacing of 2^-8 flips about one element in 10^4.
                        dxn = u |xn| + N_LN,   dq = u |xn| |w| + (1 + u) dxn |w| + N_G (|xn| |w| + |b|)
                        norms: sum_t (2 |q| dq + dq^2);   dq^ = dq + u (|q| + dq)
                        grams: sum_t (|q^| dk^ + |k^| dq^ + dq^ dk^)
      nterms == 3   xh wh + xl wh + xh wl = (xh + xl)(wh + wl) - xl wl.  The sum xh + xl follows f to S |f| (the lo part is at most
                    2^-8 |f| and is rounded to 2^-8 of itself) on either side, 2 S; the dropped xl wl is at most S |xn| |w| on either
                    side, 2 S.  The same twice for the gram.
                        dxn = 2 S |xn| + N_LN,  dq = dxn |w| + 2 S |xn| |w| + N_G (|xn| |w| + |b|)
                        norms: sum_t (2 |q| dq + dq^2);   dq~ = dq + 2 S (|q| + dq)
                        grams: sum_t (|q| dk~ + |k| dq~ + dq~ dk~ + 2 S |q| |k|)
    These bounds are wide in plain bf16 (about 1e-2 of mag) and still catch structural mistakes, because they are per block and
    relative to the block's own mag.  v in this family: nterms == 3 is held to lowprec_ref's operand-rounded bound, FP32_CHAIN_TOL of
    max(1, max|ref|), per element; nterms == 1 to the same plus the movement of the fragile LayerNorm operand elements
    (stage_ref.round_point under ln_noise, times |wh|): one flipped operand moves v by 2^-7 |xn| |w|, which is 5e-4.

chan_finish_ref.  G = the fp64 sum over blocks, mag = sum_b |partial|, constant C_REDUCE.  wbd = the fp64 softmax of
    L = G / (max(sqrt nq, 1e-12) max(sqrt nk, 1e-12)) * temperature[head]                 (csrc/fusion_ops.hip:104-108)
with a conditioning factor on the logits, as train_ref.band_mha_ref: Lmag = mag_G / (nq nk) * temperature >= |L| is the magnitude of the
logit's terms.  Counted, in units of 2^-24: the logit is off by a = 2 C_REDUCE + 5 of Lmag (C_REDUCE on G relative to mag_G; on |L|
C_REDUCE / 2 + 1 for each square root of a sum of squares, the product, the division and the temperature); t = L - max carries its own
and the maximum's error plus one rounding of |t| <= 2 Lm (Lm = the row's largest Lmag); expf costs 2; the 30-term sum at most 29 plus its
terms' error; the division 1:
    |d wbd| <= wbd * (4 a Lm + 2 * 2 Lm + 34) 2^-24 <= C_WBD 2^-24 * wbd (1 + Lm),   C_WBD = 4 a + 4 = 8 C_REDUCE + 24    (DERIVED)
so mag_wbd = wbd (1 + Lm) + FLT_MIN.  The 150 entries of a row outside its head's block have mag 0: they must be exactly 0.  Given the
bounds `dpart` of the partials (the end-to-end tests), the same chain carries them: dG += sum_b dpart, relative on the norms, through
expm1 into `extra`.

Case tables (shared by the CPU and GPU tests; each shape is the smallest at which the named path can go wrong): QKV_CASES, GRAM_CASES,
FINISH_NBLK, FINISH_IMAGES below."""
import functools
import math

import numpy as np
import torch

from attn_ref import _fixed_rows, _ints, _multiple
from lowprec_ref import FP32_CHAIN_TOL, bf16_rne, bf16_trunc, layernorm_f64
from stage_ref import GEMM_NOISE_C, ln_noise, round_point

U24 = 2.0 ** -24
FLT_MIN = 2.0 ** -126
REDUCTION_FACTOR = 4.0
HEADS, D, C = 6, 30, 180
BLK = 5760                   # floats per partial block: [6][30][30] grams, 180 q norms, 180 k norms
QKV_TOK = 256                # tokens per workgroup of chan_qkv_kernel (chan_qkv.hip:45)
CA_TOK = 32                  # tokens per LDS chunk of chan_gram_kernel (fusion_ops.hip:14)
U_BF16 = 2.0 ** -9           # the operand-rounding unit of the plain-bf16 budget
S_SPLIT = 2.0 ** -16         # the split-operand unit of the nterms == 3 budget

# measured by tests/test_chan_ref_cpu.py with the sequential fp32 stand-ins over the case tables of this module
C_GRAM_MEASURED = 17.2         # a block's gram entries: up to 257 products of both signs added one after the other
C_NORM_MEASURED = 39.8         # a block's norms: up to 257 squares, one sign (the running sum grows, and its roundings with it)
C_REDUCE_MEASURED = 6.7        # the sum over up to 57 partial blocks (FINISH_NBLK)
C_GRAM = REDUCTION_FACTOR * C_GRAM_MEASURED
C_NORM = REDUCTION_FACTOR * C_NORM_MEASURED
C_REDUCE = REDUCTION_FACTOR * C_REDUCE_MEASURED
C_PART = np.concatenate([np.full(5400, C_GRAM), np.full(360, C_NORM)])          # per element of a partial block
C_WBD = 8.0 * C_REDUCE + 24.0                                      # derived (module docstring)


# ---------------------------------------------------------------------------------------------------------------------
# the assertion
def ratios(got, ref, mag, c, extra=None):
    """|got - ref| / (c 2^-24 mag + extra) per element: 0 where got == ref, inf where got differs and the bound is 0 or got is not finite."""
    got, ref, mag = (np.asarray(a, dtype=np.float64) for a in (got, ref, mag))
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    bound = c * U24 * mag + (0.0 if extra is None else np.asarray(extra, dtype=np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got - ref)
        r = np.where(d == 0.0, 0.0, d / bound)
        r = np.where(np.isfinite(got), r, np.inf)
    return r


def check(got, ref, mag, c, what, extra=None):
    """Per-element assertion; returns the worst err / bound seen (for the reports)."""
    r = ratios(got, ref, mag, c, extra)
    worst = float(r.max()) if r.size else 0.0
    if not worst <= 1.0:
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        f = lambda a: np.asarray(a, dtype=np.float64)[i]            # noqa: E731
        raise AssertionError(f"{what}: err / bound = {worst:.3g} at {i}: got {f(got)!r}, ref {f(ref)!r}, mag {f(mag)!r}, extra "
                             f"{0.0 if extra is None else f(extra)!r}, C {np.broadcast_to(c, r.shape)[i]:g}; {int((r > 1.0).sum())} of {r.size} elements over")
    return worst


def passes(got, ref, mag, c, extra=None):
    return bool((ratios(got, ref, mag, c, extra) <= 1.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# ff_chan_qkv
def weight_planes(wqkv, bqkv):
    """The operands chan_qkv_kernel reads, taken back out of prep.pack_chan_qkv's tiles: (wh, wl [540, 180] fp64, bias [540] fp64),
    rows q | k | v."""
    from isr2_amd.prep import pack_chan_qkv
    pk = pack_chan_qkv(wqkv.float(), None if bqkv is None else bqkv.float())
    t = pk["w"].float().double().reshape(18, 2, 32, 192)
    b = pk["b"].double().reshape(18, 32)
    assert float(t[:, :, :, C:].abs().max()) == 0.0 and float(t[:12, :, D:].abs().max()) == 0.0 and float(b[:12, D:].abs().max()) == 0.0
    qk = t[:12, :, :D, :C].reshape(HEADS, 2, 2, D, C)                     # [head][q | k][plane][row][col]
    q, k = qk[:, 0].permute(1, 0, 2, 3).reshape(2, C, C), qk[:, 1].permute(1, 0, 2, 3).reshape(2, C, C)
    v = t[12:].permute(1, 0, 2, 3).reshape(2, 192, 192)[:, :C, :C]
    bq, bk = b[:12, :D].reshape(HEADS, 2, D)[:, 0].reshape(C), b[:12, :D].reshape(HEADS, 2, D)[:, 1].reshape(C)
    w = torch.cat([q, k, v], dim=1)
    return w[0], w[1], torch.cat([bq, bk, b[12:].reshape(192)[:C]])


def _blocks(t, nblk):
    """[M, 180] -> [nblk, 256, 6, 30], zero rows beyond M (chan_qkv.hip:165)."""
    pad = nblk * QKV_TOK - t.shape[0]
    if pad:
        t = torch.cat([t, t.new_zeros(pad, t.shape[1])])
    return t.reshape(nblk, QKV_TOK, HEADS, D)


def _gram(a, b):
    return torch.einsum("bthi,bthj->bhij", a, b)


def _layout(g, nq, nk):
    """[nblk, 6, 30, 30], [nblk, 6, 30] x 2 -> [nblk, 5760] (chan_qkv.hip:206-212; fusion_ops.hip:56-63)."""
    n = g.shape[0]
    return torch.cat([g.reshape(n, 5400), nq.reshape(n, C), nk.reshape(n, C)], dim=1)


def chan_qkv_blocks_ref(x, gamma, beta, wqkv, bqkv, nterms, eps, exact=False):
    """x [M, 180] fp32 -> dict(part, part_mag, part_extra [nblk, 5760], v [M, 180], v_allow [M, 180] (the movement a fragile LayerNorm
    operand allows v in plain bf16), facts).  exact: the inputs are the exact family's; the facts are filled and extra is 0."""
    assert nterms in (1, 3)
    M = x.shape[0]
    nblk = (M + QKV_TOK - 1) // QKV_TOK
    wh, wl, b = weight_planes(wqkv, bqkv)
    vln = layernorm_f64(x.float(), gamma, beta, eps)                       # chan_qkv.hip:78-104
    f = vln.float()
    xh = bf16_rne(f)                                                       # chan_qkv.hip:105-106
    xl = bf16_rne(f - xh).double()                                         # chan_qkv.hip:107
    xh = xh.double()
    _, mv_ln = round_point(vln, ln_noise(vln))
    if nterms == 1:
        proj = xh.matmul(wh.t()) + b                                       # chan_qkv.hip:133, :139
        xa, wa = xh.abs(), wh.abs()
    else:
        proj = xh.matmul(wh.t()) + xl.matmul(wh.t()) + xh.matmul(wl.t()) + b          # chan_qkv.hip:130-133, :136-139 (no lo * lo)
        xa, wa = xh.abs() + xl.abs(), wh.abs() + wl.abs()
    pmag = xa.matmul(wa.t()) + b.abs()
    facts = None
    if exact:
        gx, gw = 2.0 ** -2, 2.0 ** -5
        facts = dict(ln_move=mv_ln.max().item(), lo=max(xl.abs().max().item(), wl.abs().max().item()),
                     proj=pmag.max().item() / (2.0 ** 24 * gx * gw), grid=_multiple(xh, gx) and _multiple(wh, gw) and _multiple(b, gx * gw))
    q, k, v = proj[:, :C], proj[:, C:2 * C], proj[:, 2 * C:]               # the fp32 accumulators
    qb, kb = _blocks(q, nblk), _blocks(k, nblk)
    nq, nk = qb.pow(2).sum(1), kb.pow(2).sum(1)                            # chan_qkv.hip:166: n2 += f * f, f unrounded
    qf, kf = qb.float(), kb.float()
    qh, kh = bf16_rne(qf), bf16_rne(kf)                                    # chan_qkv.hip:167-168
    ql, kl = bf16_rne(qf - qh).double(), bf16_rne(kf - kh).double()        # chan_qkv.hip:169
    qh, kh = qh.double(), kh.double()
    if nterms == 1:
        g = _gram(qh, kh)                                                  # chan_qkv.hip:191
        gmag = _gram(qh.abs(), kh.abs())
    else:
        g = _gram(qh, kh) + _gram(qh, kl) + _gram(ql, kh)                  # chan_qkv.hip:188-191 (no lo * lo)
        gmag = _gram(qh.abs(), kh.abs()) + _gram(qh.abs(), kl.abs()) + _gram(ql.abs(), kh.abs())
    part, mag = _layout(g, nq, nk), _layout(gmag, nq, nk)
    extra = torch.zeros_like(part)
    if not exact:
        noise = GEMM_NOISE_C * U24 * pmag[:, :2 * C]
        w2 = wa[:2 * C]
        if nterms == 1:
            dxn = U_BF16 * xa + ln_noise(vln)
            dp = U_BF16 * xa.matmul(w2.t()) + (1.0 + U_BF16) * dxn.matmul(w2.t()) + noise
        else:
            dxn = 2.0 * S_SPLIT * xa + ln_noise(vln)
            dp = dxn.matmul(w2.t()) + 2.0 * S_SPLIT * xa.matmul(w2.t()) + noise
        dq, dk = _blocks(dp[:, :C], nblk), _blocks(dp[:, C:], nblk)
        qa, ka = qb.abs(), kb.abs()
        enq, enk = (2.0 * qa * dq + dq * dq).sum(1), (2.0 * ka * dk + dk * dk).sum(1)
        if nterms == 1:
            dq, dk = dq + U_BF16 * (qa + dq), dk + U_BF16 * (ka + dk)
            eg = _gram(qh.abs(), dk) + _gram(dq, kh.abs()) + _gram(dq, dk)
        else:
            dq, dk = dq + 2.0 * S_SPLIT * (qa + dq), dk + 2.0 * S_SPLIT * (ka + dk)
            eg = _gram(qa, dk) + _gram(dq, ka) + _gram(dq, dk) + 2.0 * S_SPLIT * _gram(qa, ka)
        extra = _layout(eg, enq, enk)
    v_allow = mv_ln.matmul(wh[2 * C:].abs().t()) if nterms == 1 else torch.zeros_like(v)
    return dict(part=part, part_mag=mag, part_extra=extra, v=v, v_allow=v_allow, facts=facts, nblk=nblk)


def assert_exact(facts, name):
    """The exact family's facts, from the reference alone."""
    print(f"CHAN_REF_EXACT {name}: LayerNorm movement {facts['ln_move']:.1e}, largest lo part {facts['lo']:.1e}, largest partial sum of "
          f"q / k / v / (2^24 grid steps) {facts['proj']:.2e}")
    assert facts["grid"] and facts["ln_move"] == 0.0 and facts["lo"] == 0.0 and facts["proj"] < 1.0, (name, facts)


def part_bound(mag, extra=None):
    """The absolute bound of partial blocks, as a tensor: what chan_finish_ref takes as `dpart` in the end-to-end tests."""
    b = torch.from_numpy(C_PART) * U24 * mag
    return b if extra is None else b + extra


def v_bound(res):
    """Absolute per-element bound of v in the correlated family."""
    return FP32_CHAIN_TOL * max(1.0, res["v"].abs().max().item()) + res["v_allow"]


# ---------------------------------------------------------------------------------------------------------------------
# chan_gram_kernel
def gram_plan(N):
    """ff_chan_attn_weights' host rule (fusion_ops.hip:134-137) -> (nblk, tok_per_blk)."""
    nblk = min((N + 255) // 256, 1024)
    tpb = (N + nblk - 1) // nblk
    return (N + tpb - 1) // tpb, tpb


def chan_gram_blocks_ref(qkv, q_off, k_off, N):
    """qkv [N, ld] fp32 -> (part, mag [nblk, 5760]): block b holds tokens b tpb .. min(N, (b + 1) tpb) - 1 (fusion_ops.hip:26-28)."""
    nblk, tpb = gram_plan(N)
    part = torch.zeros(nblk, BLK, dtype=torch.float64)
    mag = torch.zeros(nblk, BLK, dtype=torch.float64)
    step = max(1, 32768 // tpb)
    for b0 in range(0, nblk, step):
        b1 = min(nblk, b0 + step)
        rows = qkv[b0 * tpb:min(N, b1 * tpb)]
        q, k = rows[:, q_off:q_off + C].double(), rows[:, k_off:k_off + C].double()
        pad = (b1 - b0) * tpb - rows.shape[0]
        if pad:
            q, k = torch.cat([q, q.new_zeros(pad, C)]), torch.cat([k, k.new_zeros(pad, C)])
        q, k = q.reshape(b1 - b0, tpb, HEADS, D), k.reshape(b1 - b0, tpb, HEADS, D)
        nq, nk = q.pow(2).sum(1), k.pow(2).sum(1)                          # fusion_ops.hip:50-51
        part[b0:b1] = _layout(_gram(q, k), nq, nk)                         # fusion_ops.hip:49
        mag[b0:b1] = _layout(_gram(q.abs(), k.abs()), nq, nk)
    return part, mag


# ---------------------------------------------------------------------------------------------------------------------
# chan_reduce_body + chan_attn_weights_body
def chan_finish_ref(partials, temperature, dpart=None):
    """partials [nblk, 5760] (the fp32 values the kernels read, or a reference's), temperature [6]; dpart: absolute bounds of the
    partials or None -> dict(G, G_mag, G_extra [5760], wbd, wbd_mag, wbd_extra [180, 180], spread = the largest logit range of a row)."""
    p = torch.as_tensor(partials).double()
    temp = torch.as_tensor(temperature).double()
    G, Gmag = p.sum(0), p.abs().sum(0)                                     # fusion_ops.hip:74-87
    dG = torch.zeros_like(G) if dpart is None else torch.as_tensor(dpart).double().sum(0)
    g, gm, dg = G[:5400].reshape(HEADS, D, D), Gmag[:5400].reshape(HEADS, D, D), dG[:5400].reshape(HEADS, D, D)
    n2q, n2k = G[5400:5580].reshape(HEADS, D, 1), G[5580:].reshape(HEADS, 1, D)
    dnq, dnk = dG[5400:5580].reshape(HEADS, D, 1), dG[5580:].reshape(HEADS, 1, D)
    nq, nk = n2q.sqrt().clamp_min(1e-12), n2k.sqrt().clamp_min(1e-12)      # fusion_ops.hip:104, :107
    t = temp.reshape(HEADS, 1, 1)
    L = g / (nq * nk) * t                                                  # fusion_ops.hip:108
    Lmag = gm / (nq * nk) * t
    Lm = Lmag.amax(-1, keepdim=True)
    wbd_h = torch.softmax(L, dim=-1)                                       # fusion_ops.hip:111-116
    spread = (L.amax(-1) - L.amin(-1)).max().item()
    rel = lambda d, n: torch.where(d > 0, 0.5 * d / (n - d).clamp_min(1e-300), torch.zeros_like(d))       # noqa: E731  (of a square root)
    r = rel(dnq, n2q) + rel(dnk, n2k)
    dL = (dg / (nq * nk) * t + L.abs() * r) * (1.0 + 2.0 * r)
    ex_h = wbd_h * torch.expm1(dL + 3.0 * dL.amax(-1, keepdim=True))
    wbd = torch.zeros(C, C, dtype=torch.float64)
    wmag, wex = torch.zeros_like(wbd), torch.zeros_like(wbd)
    for h in range(HEADS):
        s = slice(h * D, (h + 1) * D)
        wbd[s, s], wmag[s, s], wex[s, s] = wbd_h[h], wbd_h[h] * (1.0 + Lm[h]) + FLT_MIN, ex_h[h]
    return dict(G=G, G_mag=Gmag, G_extra=dG, wbd=wbd, wbd_mag=wmag, wbd_extra=wex, spread=spread)


# ---------------------------------------------------------------------------------------------------------------------
# cases and inputs (seeded CPU generators; CPU tensors, the GPU test moves them)
# ff_chan_qkv: M = 77: wave 2 ragged with 13 live tokens, waves 3 .. 7 all masked; 256: one full block; 257: the second block holds one
# token; 3000; 8192 + 31; ld = 192: NaN in columns 180 .. 191 of x, a sentinel in the same columns of v.  65536 (the bench size) once.
QKV_SHAPES = [dict(M=77, ld=180), dict(M=256, ld=192), dict(M=257, ld=180), dict(M=3000, ld=192), dict(M=8192 + 31, ld=180)]
QKV_CASES = ([dict(s, family=fam, nterms=n) for fam in ("exact", "corr") for n in (1, 3) for s in QKV_SHAPES]
             + [dict(M=65536, ld=180, family="corr", nterms=1)])
# chan_gram_kernel: N = 31 < CA_TOK; 256; 257; 3000; 262144 + 37: nblk capped at 1024 and tok_per_blk = 257, no multiple of 32;
# ld > 540 with NaN outside the q and k slices
GRAM_CASES = [dict(N=31, ld=540, q_off=0, k_off=180), dict(N=256, ld=540, q_off=0, k_off=180), dict(N=257, ld=548, q_off=4, k_off=364),
              dict(N=3000, ld=548, q_off=4, k_off=364), dict(N=262144 + 37, ld=360, q_off=0, k_off=180)]
# chan_reduce_body: the 4-way unrolled loop `b + 24 < nblk`, its stride-8 tail, slices with no block at all
FINISH_NBLK = [1, 7, 8, 9, 31, 32, 33, 57]
FINISH_IMAGES = [dict(B=3, nblk=1), dict(B=3, nblk=9)]
TEMPERATURE = [0.5, 1.0, 2.0, 4.0, 8.0, 1.5]
ZERO_Q, ZERO_K = 37, 95                                                   # finish cases: a q and a k channel whose norm is exactly 0


def case_name(case):
    return "-".join(f"{k}{v}" for k, v in case.items())


def _randn(*shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def corr_weights(seed):
    """wqkv [540, 180], bqkv [540]: k channel 30 h + i = 0.8 s_i * q channel 30 h + pi_h(i) + 0.6 noise."""
    wq, wv = _randn(C, C, seed=seed, scale=C ** -0.5), _randn(C, C, seed=seed + 1, scale=C ** -0.5)
    noise = _randn(C, C, seed=seed + 2, scale=C ** -0.5)
    g = torch.Generator(device="cpu").manual_seed(seed + 3)
    perm = torch.cat([h * D + torch.randperm(D, generator=g) for h in range(HEADS)])
    sign = torch.randint(0, 2, (C, 1), generator=g).float() * 2.0 - 1.0
    wk = 0.8 * sign * wq[perm] + 0.6 * noise
    return torch.cat([wq, wk, wv]), _randn(3 * C, seed=seed + 4, scale=0.1), perm, sign[:, 0]


def qkv_inputs(M, family, seed=None):
    """-> dict(x [M, 180], gamma, beta, wqkv, bqkv, eps)."""
    seed = 4100 + M if seed is None else seed
    if family == "exact":
        betas = torch.tensor([0.0, 1.25, -1.25, 1.75, -1.75, 2.5, -2.5])   # attn_ref.make_inputs: beta never cancels x * gamma
        return dict(x=_fixed_rows(M, C, seed), gamma=torch.tensor([0.5, 1.0, 2.0])[_ints(C, lo=0, hi=2, seed=seed + 1).long()],
                    beta=betas[_ints(C, lo=0, hi=6, seed=seed + 2).long()], wqkv=_ints(3 * C, C, lo=-2, hi=2, seed=seed + 3) / 32.0,
                    bqkv=_ints(3 * C, lo=-8, hi=8, seed=seed + 4) / 16.0, eps=0.0)
    wqkv, bqkv, _, _ = corr_weights(seed + 10)
    x = _randn(M, C, seed=seed, scale=1.5) + 0.3
    nt = min(32, M)
    g = torch.Generator(device="cpu").manual_seed(seed + 5)
    rows = torch.randint(0, C, (nt, 3), generator=g)
    x[M - nt:] = 4.0 * (wqkv[:C][rows].sum(1) * math.sqrt(C) + _randn(nt, C, seed=seed + 6, scale=0.3))
    return dict(x=x, gamma=_randn(C, seed=seed + 7, scale=0.1) + 1.0, beta=_randn(C, seed=seed + 8, scale=0.1), wqkv=wqkv, bqkv=bqkv, eps=1e-5)


@functools.lru_cache(maxsize=None)
def qkv_reference(M, family, nterms):
    """-> (inputs, chan_qkv_blocks_ref's dict), computed once per case and shared (callers leave them unchanged)."""
    inp = qkv_inputs(M, family)
    return inp, chan_qkv_blocks_ref(nterms=nterms, exact=family == "exact", **inp)


def gram_inputs(N, ld, q_off, k_off, seed=None):
    """qkv [N, ld] fp32: q = randn, k follows a signed permutation of q's channels (0.8 q + 0.6 noise), NaN outside the two slices."""
    seed = 4300 + N % 100003 if seed is None else seed
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.randn(N, C, generator=g)
    perm = torch.cat([h * D + torch.randperm(D, generator=g) for h in range(HEADS)])
    sign = torch.randint(0, 2, (C,), generator=g).float() * 2.0 - 1.0
    k = torch.randn(N, C, generator=g).mul_(0.6).add_(q[:, perm] * (0.8 * sign))
    qkv = torch.full((N, ld), float("nan"))
    qkv[:, q_off:q_off + C], qkv[:, k_off:k_off + C] = q, k
    return qkv


@functools.lru_cache(maxsize=None)
def gram_reference(N, ld, q_off, k_off):
    qkv = gram_inputs(N, ld, q_off, k_off)
    return qkv, chan_gram_blocks_ref(qkv, q_off, k_off, N)


def finish_inputs(nblk, seed=None):
    """Synthetic partials [nblk, 5760] fp32 with mixed signs: per head a cosine matrix in [-0.8, 0.8] (head 4, at temperature 8, holds
    +0.8 and -0.8 in every row: a logit spread of 12.8), norms^2 in [2500, 22500], split over the blocks with weights of both signs
    (grams) or positive weights (norms).  q channel ZERO_Q and k channel ZERO_K have norm exactly 0 and an all-zero gram row / column."""
    seed = 4500 + nblk if seed is None else seed
    g = torch.Generator(device="cpu").manual_seed(seed)
    cos = torch.rand(HEADS, D, D, generator=g, dtype=torch.float64) * 1.6 - 0.8
    j = torch.arange(D)
    cos[4, j, (j * 7 + 3) % D], cos[4, j, (j * 7 + 4) % D] = 0.8, -0.8
    nq = torch.rand(HEADS, D, generator=g, dtype=torch.float64) * 100.0 + 50.0
    nk = torch.rand(HEADS, D, generator=g, dtype=torch.float64) * 100.0 + 50.0
    nq.reshape(-1)[ZERO_Q], nk.reshape(-1)[ZERO_K] = 0.0, 0.0
    tot = torch.cat([(cos * nq[:, :, None] * nk[:, None, :]).reshape(-1), nq.reshape(-1) ** 2, nk.reshape(-1) ** 2])
    wg = torch.randn(nblk, BLK, generator=g, dtype=torch.float64) * 0.75 + 1.0          # about one in eleven is negative
    wn = torch.rand(nblk, BLK, generator=g, dtype=torch.float64) + 0.5
    wt = torch.cat([wg[:, :5400], wn[:, 5400:]], dim=1)
    wt = wt / wt.sum(0, keepdim=True).abs().clamp_min(0.25)
    return (wt * tot).float()


@functools.lru_cache(maxsize=None)
def finish_reference(nblk, seed=None):
    p = finish_inputs(nblk, seed)
    return p, chan_finish_ref(p, TEMPERATURE)

