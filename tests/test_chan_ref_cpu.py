"""CPU checks of tests/golden/chan_ref.py, the references tests/test_chan_attn_gpu.py holds DAT's channel attention to.  No GPU: a
stand-in plays each kernel's arithmetic in fp32 -- the same fp32 products, summed STRICTLY SEQUENTIALLY in token (block) order -- over
the case tables of chan_ref (the GPU test imports the same tables).

  * the stand-ins pass every per-element assertion of the module, in both families and both nterms;
  * the exact family's facts hold for every exact case (zero LayerNorm movement, zero lo parts, partial sums below 2^24 grid steps),
    and the stand-in's v is bit-equal there;
  * the constants are re-measured: the worst |stand-in - ref| / (2^-24 mag) stays within *_MEASURED * 1.25, the module's constants
    equal 4 * *_MEASURED, and the counted C_WBD covers the stand-in;
  * fp64 PyTorch (F.normalize, softmax: the formula of the model) agrees with chan_finish_ref of chan_gram_blocks_ref to 1e-12 * mag;
  * every mutant of a stand-in FAILS the assertion in every case it applies to.  A mutant the assertion cannot tell from the stand-in
    is reported by name and fails the test unless UNDETECTABLE lists it with its reason.

Mutants (family: name -- where it applies):
    qkv: drop_token (the last live token), drop_wave (the 32-token wave holding it), mask_off1 (`tok <= M`: M % 256 != 0), k_norm_q
         (k norms taken from q), transposed, neighbour (a block written to the next slot: nblk > 1) -- both families;
         norm_rounded (norms from the rounded q), trunc (truncation at (__bf16)q: nterms 1), lolo (lo * lo kept: nterms 3), no_hilo
         (hi * lo dropped: nterms 3) -- the exact family: these move a partial by 2^-9 .. 2^-18 of its mag, which the correlated
         family's forward bound (1e-2 of mag in plain bf16, 1e-3 in split bf16) is too wide to see, by construction.
    gram: drop_token, drop_chunk (the last 32-token LDS chunk of the last block), k_norm_q, transposed, neighbour (nblk > 1)
    finish: no_tail (chan_reduce without its stride-8 tail loop: every nblk but 32, which the unrolled loop covers alone), temp_head (the
         next head's temperature), no_clamp (no 1e-12 clamp: 0 / 0), offblock (a nonzero entry outside a head's block)
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import chan_ref as R  # noqa: E402
from lowprec_ref import bf16_rne, bf16_trunc, chunked_fp32_matmul  # noqa: E402
from stage_ref import layernorm_fp32  # noqa: E402

# (family, mutant) -> why the assertion cannot see it
UNDETECTABLE = {
    ("qkv:exact3", "lolo"): "a lo part is at most 2^-9 of its value, so lo * lo is at most 2^-18 of |q||k| per term, of either sign: the "
                            "size of the fp32 summation bound C_GRAM 2^-24 itself -- which is why the kernel may drop the term",
    ("qkv:corr1", "mask_off1"): "token M is the LayerNorm of a zero row, beta W + b with |beta| about 0.1: its q k products are 1e-3 of a "
                                "typical token's, under the 1e-2 of mag of the plain-bf16 forward bound; the exact family (|beta| up to "
                                "2.5) and split bf16 see it in every case",
}
WORST = {}
f32 = torch.float32


def note(key, r):
    WORST[key] = max(WORST.get(key, 0.0), r)
    return r


def measure(part, ref, mag):
    """|stand-in - ref| / (2^-24 mag) of a block's gram entries and of its norms."""
    r = R.ratios(part.numpy(), ref.numpy(), mag.numpy(), 1.0)
    return note("gram", float(r[:, :5400].max())), note("norm", float(r[:, 5400:].max()))


def seq_sum(terms):
    """Strictly sequential fp32 sum along axis 1 of terms [n, T, ...] (fp32 products)."""
    acc = torch.zeros_like(terms[:, 0])
    for t in range(terms.shape[1]):
        acc = acc + terms[:, t]
    return acc


def seq_gram(*pairs):
    """sum_t a[:, t, h, i] b[:, t, h, j], every product an fp32 number, added one token after the other -> [n, 6, 30, 30]."""
    a0 = pairs[0][0]
    acc = torch.zeros(a0.shape[0], R.HEADS, R.D, R.D, dtype=f32)
    for t in range(a0.shape[1]):
        for a, b in pairs:
            acc = acc + a[:, t, :, :, None] * b[:, t, :, None, :]
    return acc


def _fails(family, mutant, case, ok, undetected):
    if ok and (family, mutant) not in UNDETECTABLE:
        undetected.append(f"{family}:{mutant}@{case}")


# ---------------------------------------------------------------------------------------------------------------------
# ff_chan_qkv
QKV_MUT_BOTH = ("drop_token", "drop_wave", "mask_off1", "k_norm_q", "transposed", "neighbour")
QKV_MUT_EXACT = ("norm_rounded", "trunc", "lolo", "no_hilo")


def qkv_standin(inp, nterms, mut=None):
    x = inp["x"].float()
    M = x.shape[0]
    nblk = (M + 255) // 256
    wh, wl, b = (t.float() for t in R.weight_planes(inp["wqkv"], inp["bqkv"]))
    xp = torch.cat([x, torch.zeros(nblk * 256 - M, R.C)])                  # rows beyond M are loaded as zeros: their LayerNorm is beta
    f = layernorm_fp32(xp, inp["gamma"], inp["beta"], inp["eps"])
    f[M:] = inp["beta"].float()
    xh = bf16_rne(f)
    xl = bf16_rne(f - xh)
    proj = chunked_fp32_matmul(xh, wh)
    if nterms == 3:
        proj = proj + chunked_fp32_matmul(xl, wh) + chunked_fp32_matmul(xh, wl)
    proj = proj + b
    v = proj[:M, 2 * R.C:]
    live = torch.arange(nblk * 256) < (M + 1 if mut == "mask_off1" else M)
    if mut == "drop_token":
        live[M - 1] = False
    if mut == "drop_wave":
        live[(M - 1) // 32 * 32:] = False
    qk = torch.where(live[:, None], proj[:, :2 * R.C], torch.zeros((), dtype=f32))
    q, k = qk[:, :R.C].reshape(nblk, 256, R.HEADS, R.D), qk[:, R.C:].reshape(nblk, 256, R.HEADS, R.D)
    rn = bf16_trunc if mut == "trunc" else bf16_rne
    qh, kh = rn(q), rn(k)
    ql, kl = bf16_rne(q - qh), bf16_rne(k - kh)
    nsrc_q, nsrc_k = (qh, kh) if mut == "norm_rounded" else (q, k)
    nq, nk = seq_sum(nsrc_q * nsrc_q), seq_sum(nsrc_k * nsrc_k)
    if mut == "k_norm_q":
        nk = nq
    pairs = [(qh, kh)]
    if nterms == 3:
        pairs = [(qh, kl), (ql, kh), (qh, kh)]
        if mut == "lolo":
            pairs.append((ql, kl))
        if mut == "no_hilo":
            pairs = pairs[1:]
    g = seq_gram(*pairs)
    if mut == "transposed":
        g = g.transpose(-1, -2)
    part = R._layout(g, nq, nk)
    if mut == "neighbour":
        part = part.roll(1, 0)
    return part, v


def _qkv_applies(mut, case):
    M, nblk = case["M"], (case["M"] + 255) // 256
    if mut == "mask_off1":
        return M % 256 != 0
    if mut == "neighbour":
        return nblk > 1
    if mut == "trunc":
        return case["nterms"] == 1
    if mut in ("lolo", "no_hilo"):
        return case["nterms"] == 3
    return True


@pytest.mark.parametrize("case", R.QKV_CASES, ids=R.case_name)
def test_chan_qkv_standin_and_mutants(case):
    M, fam, nterms = case["M"], case["family"], case["nterms"]
    inp, ref = R.qkv_reference(M, fam, nterms)
    part, v = qkv_standin(inp, nterms)
    assert part.shape == (ref["nblk"], R.BLK)
    args = (ref["part"].numpy(), ref["part_mag"].numpy(), R.C_PART)
    extra = ref["part_extra"].numpy()
    name = R.case_name(case)
    if fam == "exact":
        R.assert_exact(ref["facts"], name)
        assert float(ref["part_extra"].abs().max()) == 0.0
        assert torch.equal(v.double(), ref["v"]), "v of the exact family is not bit-equal"
        # the measurement: the exact family's partials differ from the reference by the summation order alone
        measure(part, ref["part"], ref["part_mag"])
    else:
        bound = R.v_bound(ref)
        assert bool(((v.double() - ref["v"]).abs() <= bound).all()), "v outside the operand-rounded bound"
    r = R.check(part.numpy(), *args, f"stand-in {name}", extra)
    print(f"CHAN_REF_CPU qkv {name}: stand-in err / bound {r:.3f}")
    undetected = []
    for mut in QKV_MUT_BOTH + (QKV_MUT_EXACT if fam == "exact" else ()):
        if _qkv_applies(mut, case) and not (M == 65536 and mut not in ("drop_wave", "transposed")):     # the bench size: two mutants, for time
            mp, _ = qkv_standin(inp, nterms, mut)
            _fails(f"qkv:{fam}{nterms}", mut, name, R.passes(mp.numpy(), *args, extra), undetected)
    assert not undetected, undetected


# ---------------------------------------------------------------------------------------------------------------------
# chan_gram_kernel
GRAM_MUT = ("drop_token", "drop_chunk", "k_norm_q", "transposed", "neighbour")


def gram_standin(qkv, q_off, k_off, N, mut=None):
    nblk, tpb = R.gram_plan(N)
    q, k = qkv[:, q_off:q_off + R.C].clone(), qkv[:, k_off:k_off + R.C].clone()
    if mut == "drop_token":
        q[N - 1], k[N - 1] = 0.0, 0.0
    if mut == "drop_chunk":
        first = (nblk - 1) * tpb
        cut = first + (N - 1 - first) // R.CA_TOK * R.CA_TOK
        q[cut:], k[cut:] = 0.0, 0.0
    pad = torch.zeros(nblk * tpb - N, R.C)
    q, k = torch.cat([q, pad]).reshape(nblk, tpb, R.HEADS, R.D), torch.cat([k, pad]).reshape(nblk, tpb, R.HEADS, R.D)
    nq, nk = seq_sum(q * q), seq_sum(k * k)
    if mut == "k_norm_q":
        nk = nq
    g = seq_gram((q, k))
    if mut == "transposed":
        g = g.transpose(-1, -2)
    part = R._layout(g, nq, nk)
    return part.roll(1, 0) if mut == "neighbour" else part


@pytest.mark.parametrize("case", R.GRAM_CASES, ids=R.case_name)
def test_chan_gram_standin_and_mutants(case):
    N = case["N"]
    qkv, (ref, mag) = R.gram_reference(**case)
    nblk, tpb = R.gram_plan(N)
    assert ref.shape == (nblk, R.BLK) and nblk <= 1024 and (nblk - 1) * tpb < N <= nblk * tpb
    if N == 262144 + 37:
        assert (nblk, tpb) == (1021, 257)                                  # 1024 blocks of 257 tokens would pass N: the host rule's second line
    part = gram_standin(qkv, case["q_off"], case["k_off"], N)
    name = R.case_name(case)
    R.check(part.numpy(), ref.numpy(), mag.numpy(), R.C_PART, f"stand-in {name}")
    rg, rn = measure(part, ref, mag)
    print(f"CHAN_REF_CPU gram {name}: stand-in |d| / (2^-24 mag): grams {rg:.2f}, norms {rn:.2f}")
    undetected = []
    for mut in GRAM_MUT:
        if (mut != "neighbour" or nblk > 1) and not (N > 100000 and mut not in ("drop_token", "transposed")):
            mp = gram_standin(qkv, case["q_off"], case["k_off"], N, mut)
            _fails("gram", mut, name, R.passes(mp.numpy(), ref.numpy(), mag.numpy(), R.C_PART), undetected)
    assert not undetected, undetected


# ---------------------------------------------------------------------------------------------------------------------
# chan_reduce_body + chan_attn_weights_body
FINISH_MUT = ("no_tail", "temp_head", "no_clamp", "offblock")


def tail_blocks(nblk):
    """The blocks chan_reduce_body's stride-8 tail loop sums (fusion_ops.hip:80): those its unrolled loop leaves."""
    left = set(range(nblk))
    for sl in range(8):
        b = sl
        while b + 24 < nblk:
            left -= {b, b + 8, b + 16, b + 24}
            b += 32
    return sorted(left)


def finish_standin(p, temperature, mut=None):
    p = p.float()
    if mut == "no_tail":
        p = p.clone()
        p[tail_blocks(p.shape[0])] = 0.0
    G = seq_sum(p[None])[0]
    temp = torch.tensor(temperature, dtype=f32)
    if mut == "temp_head":
        temp = temp.roll(-1)
    g = G[:5400].reshape(R.HEADS, R.D, R.D)
    nq, nk = G[5400:5580].reshape(R.HEADS, R.D, 1).sqrt(), G[5580:].reshape(R.HEADS, 1, R.D).sqrt()
    if mut != "no_clamp":
        nq, nk = nq.clamp_min(1e-12), nk.clamp_min(1e-12)
    L = g / (nq * nk) * temp.reshape(R.HEADS, 1, 1)
    e = torch.exp(L - L.amax(-1, keepdim=True))
    s = seq_sum(e.reshape(-1, R.D))
    w = e / s.reshape(R.HEADS, R.D, 1)
    wbd = torch.zeros(R.C, R.C, dtype=f32)
    for h in range(R.HEADS):
        wbd[h * R.D:(h + 1) * R.D, h * R.D:(h + 1) * R.D] = w[h]
    if mut == "offblock":
        wbd[0, R.C - 1] = 1e-30
    return G, wbd


@pytest.mark.parametrize("nblk", R.FINISH_NBLK)
def test_chan_finish_standin_and_mutants(nblk):
    p, ref = R.finish_reference(nblk)
    assert bool((p[:, :5400] < 0).any()) and bool((p[:, :5400] > 0).any()), "partials of one sign"
    assert ref["spread"] > 10.0, ref["spread"]
    z = ref["wbd"][R.ZERO_Q, R.ZERO_Q // R.D * R.D:(R.ZERO_Q // R.D + 1) * R.D]
    assert bool((z == 1.0 / R.D).all()) or float((z - 1.0 / R.D).abs().max()) < 1e-16, "a zero-norm q channel gives a uniform row"
    assert float(ref["wbd_mag"][0, R.D:].max()) == 0.0 and float(ref["wbd_extra"].max()) == 0.0
    G, wbd = finish_standin(p, R.TEMPERATURE)
    rg = note("reduce", R.check(G.numpy(), ref["G"].numpy(), ref["G_mag"].numpy(), R.C_REDUCE, f"stand-in G nblk={nblk}") * R.C_REDUCE)
    rw = note("wbd", R.check(wbd.numpy(), ref["wbd"].numpy(), ref["wbd_mag"].numpy(), R.C_WBD, f"stand-in wbd nblk={nblk}") * R.C_WBD)
    print(f"CHAN_REF_CPU finish nblk={nblk}: stand-in |d| / (2^-24 mag): G {rg:.2f}, wbd {rw:.2f}; logit spread {ref['spread']:.1f}")
    undetected = []
    for mut in FINISH_MUT:
        if mut == "no_tail" and not tail_blocks(nblk):
            assert nblk == 32
            continue
        mG, mw = finish_standin(p, R.TEMPERATURE, mut)
        ok = R.passes(mG.numpy(), ref["G"].numpy(), ref["G_mag"].numpy(), R.C_REDUCE) and \
            R.passes(mw.numpy(), ref["wbd"].numpy(), ref["wbd_mag"].numpy(), R.C_WBD)
        _fails("finish", mut, f"nblk={nblk}", ok, undetected)
    assert not undetected, undetected


def test_finish_reference_is_the_models_formula():
    """dat_arch.py's channel attention in fp64 PyTorch: q, k [heads, d, N] L2-normalised over the tokens, (q @ k^T) * temperature, softmax."""
    case = R.GRAM_CASES[3]
    qkv, (part, _) = R.gram_reference(**case)
    N = case["N"]
    q = qkv[:, case["q_off"]:case["q_off"] + R.C].double().t().reshape(R.HEADS, R.D, N)
    k = qkv[:, case["k_off"]:case["k_off"] + R.C].double().t().reshape(R.HEADS, R.D, N)
    attn = (F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-1, -2)) * torch.tensor(R.TEMPERATURE, dtype=torch.float64).reshape(-1, 1, 1)
    want = torch.block_diag(*attn.softmax(-1))
    ref = R.chan_finish_ref(part, R.TEMPERATURE)
    assert bool(((want - ref["wbd"]).abs() <= 1e-12 * ref["wbd_mag"]).all())
    gq = torch.einsum("hin,hjn->hij", q, k).reshape(-1)
    assert bool(((gq - ref["G"][:5400]).abs() <= 1e-12 * ref["G_mag"][:5400]).all())
    # the end-to-end bound with no bound on the partials is no bound at all
    assert float(ref["wbd_extra"].max()) == 0.0
    wide = R.chan_finish_ref(part, R.TEMPERATURE, dpart=R.part_bound(part.abs()) + 1e-3 * part.abs())
    assert float(wide["wbd_extra"].max()) > 0.0 and float(wide["wbd_extra"][0, R.D:].max()) == 0.0


def test_correlated_inputs_are_correlated():
    """The family's point: cosines up to about 0.8, peaked softmax rows, and a tail wave that weighs in its block."""
    inp, ref = R.qkv_reference(3000, "corr", 3)
    fin = R.chan_finish_ref(ref["part"], R.TEMPERATURE)
    G = fin["G"]
    cos = G[:5400].reshape(R.HEADS, R.D, R.D) / (G[5400:5580].reshape(R.HEADS, R.D, 1).sqrt() * G[5580:].reshape(R.HEADS, 1, R.D).sqrt())
    assert cos.abs().max().item() > 0.7, cos.abs().max().item()
    assert fin["wbd"].max().item() > 0.5 and fin["spread"] > 5.0, (fin["wbd"].max().item(), fin["spread"])
    last = ref["part_mag"][-1, 5400:5580].sum().item()               # the last block holds 184 tokens; its last wave the 24 built ones
    assert last > 0.0
    x = inp["x"].clone()
    assert x[-32:].abs().mean().item() > 3.0 * x[:-32].abs().mean().item()


def test_constants_are_the_measured_ones():
    """Runs after the stand-in tests of this module (pytest keeps file order): WORST holds their measurements."""
    assert R.C_GRAM == R.REDUCTION_FACTOR * R.C_GRAM_MEASURED and R.C_NORM == R.REDUCTION_FACTOR * R.C_NORM_MEASURED
    assert R.C_REDUCE == R.REDUCTION_FACTOR * R.C_REDUCE_MEASURED
    assert R.C_WBD == 8.0 * R.C_REDUCE + 24.0
    if {"gram", "norm", "reduce", "wbd"} <= set(WORST):
        print(f"CHAN_REF_CPU measured: gram {WORST['gram']:.2f} (recorded {R.C_GRAM_MEASURED}), norm {WORST['norm']:.2f} (recorded "
              f"{R.C_NORM_MEASURED}), reduce {WORST['reduce']:.2f} (recorded {R.C_REDUCE_MEASURED}), wbd {WORST['wbd']:.2f} of the counted {R.C_WBD:g}")
        for key, rec in (("gram", R.C_GRAM_MEASURED), ("norm", R.C_NORM_MEASURED), ("reduce", R.C_REDUCE_MEASURED)):
            assert 0.5 * rec <= WORST[key] <= 1.25 * rec, (key, WORST[key], rec)
