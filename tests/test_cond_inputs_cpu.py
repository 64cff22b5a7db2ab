"""CPU checks of tests/golden/cond_inputs.py: every input family has the property it is named for, the fp32 stand-in of every chain stays
within STANDIN_CAP of fp64 on every family (so the families are inside what fp32 arithmetic can do), and the statistics bar of
tests/test_conditioning_gpu.py separates the one-pass variance from the two-pass-grade forms without a GPU."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import cond_inputs as ci  # noqa: E402

F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("M,C", [(77, 180), (77, 64), (109, 1024), (153, 64)])
def test_layernorm_families_have_their_properties(M, C):
    x, fam = ci.ln_rows(M, C, seed=1)
    assert x.shape == (M, C) and x.dtype == F32 and M % 32 != 0, "the last 32-row tile must be ragged"
    assert len(ci.ln_rows(M, C, seed=1, skip=("offset_1000_1",))[1]) == len(fam) - 1
    assert [n for n, _ in ci.FAMILIES] == list(fam) and "lowvar_5" not in fam and sum(s.stop - s.start for s in fam.values()) == M
    for name, (kind, m, s) in ci.FAMILIES:
        b = x[fam[name]].double()
        assert b.shape[0] >= 2
        if kind == "randn":
            sd = b.std(-1, unbiased=False).mean().item()
            assert abs(sd / s - 1) < 0.1, (name, sd)
            if m != 0:
                ratio = (b.mean(-1) / b.std(-1, unbiased=False)).mean().item()
                assert abs(ratio / (m / s) - 1) < 0.1, (name, ratio)
            else:
                assert abs(b.mean().item()) < 4 * s / b.numel() ** 0.5, name
        elif kind == "const":
            assert (b == float(torch.tensor(m, dtype=F32))).all()
        else:
            assert ((b != 0).sum(-1) == 1).all() and (b.max(-1).values == m).all()
    # const 3.0: the fp32 sum is exact in any order, so mean == 3 and x - mean == 0 exactly; const 0.1: it is not
    c3 = x[fam["const_3"]]
    s = torch.zeros(c3.shape[0])
    for j in range(C):
        s = s + c3[:, j]
    assert (s == 3.0 * C).all() and (c3.sum(-1) == 3.0 * C).all() and (s / C == 3.0).all()
    g, b = ci.ln_params(C, 7)
    assert torch.equal(ci.layernorm(c3, g, b, 1e-5, F32), b.expand(c3.shape[0], C))
    # const 0.1: a running fp32 sum is NOT exact, so mean != 0.1f and x - mean != 0 (what the kernels' lane sums see)
    c01 = x[fam["const_0.1"]]
    s = torch.zeros(c01.shape[0])
    for j in range(C):
        s = s + c01[:, j]
    assert (s / C != c01[:, 0]).all(), "the running sum of the 0.1 block came out exact"
    # lowvar: the variance is comparable with eps
    for name in ("lowvar_0",):
        var = x[fam[name]].double().var(-1, unbiased=False).mean().item()
        assert 0.5e-6 < var < 2e-6, (name, var)


def _chains():
    """name -> (fn(dtype) -> tensor or tuple of tensors [M, ...], fam).  The shapes of tests/test_conditioning_gpu.py."""
    out = {}
    for C, eps in ((180, 1e-5), (64, 1e-6), (1024, 1e-6)):
        x, fam = ci.ln_rows(77 if C != 1024 else 109, C, seed=2)
        g, b = ci.ln_params(C, 10)
        out[f"layernorm C={C}"] = (lambda dt, x=x, g=g, b=b, eps=eps: ci.layernorm(x, g, b, eps, dt), fam)
    for K, N in ((180, 180), (64, 128)):
        x, fam = ci.ln_rows(77, K, seed=3)
        g, b = ci.ln_params(K, 20)
        w, bias = ci.lin_params(N, K, 22)
        eps = 1e-5 if K == 180 else 1e-6
        out[f"token_linear K={K}"] = (lambda dt, x=x, g=g, b=b, w=w, bias=bias, eps=eps: ci.token_linear(x, g, b, eps, w, bias, "gelu", dt), fam)
    x, fam = ci.ln_rows(77, 180, seed=4)
    g, b = ci.ln_params(180, 30)
    w1, b1 = ci.lin_params(360, 180, 32)
    w2, b2 = ci.lin_params(180, 360, 34)
    out["token_mlp"] = (lambda dt: ci.token_mlp(x, g, b, w1, b1, w2, b2, dt), fam)
    att = ci.rnd(77, 180, seed=36)
    wp, bp = ci.lin_params(180, 180, 37)
    out["token_projmlp"] = (lambda dt: ci.token_projmlp(att, x, wp, bp, w1, b1, w2, b2, g, b, dt), fam)
    y, famn = ci.ln_rows(77, 64, seed=5)
    gn, bn = ci.ln_params(64, 40)
    w4, b4 = ci.lin_params(128, 64, 42)
    w5, b5 = ci.lin_params(64, 64, 44)
    gam = ci.rnd(64, seed=46, scale=0.3)
    out["naf_ffn"] = (lambda dt: ci.naf_ffn(y, gn, bn, w4, b4, w5, b5, gam, dt), famn)
    xi, fami = ci.ln_rows(153, 64, seed=6)
    wd, bd = ci.rnd(128, 1, 3, 3, seed=47, scale=0.3), ci.rnd(128, seed=48, scale=0.1)
    out["naf_front"] = (lambda dt: ci.naf_front(xi.reshape(9, 17, 64), gn, bn, w4, b4, wd, bd, dt)[0].reshape(153, 64), fami)
    out["naf_front pool"] = (lambda dt: ci.naf_front(xi.reshape(9, 17, 64), gn, bn, w4, b4, wd, bd, dt)[1].reshape(1, 64), ci.ALL)
    gt = ci.rnd(77, 64, seed=140)
    w3, b3 = ci.lin_params(64, 64, 141)
    sca, beta = ci.rnd(64, seed=143) * 0.3 + 1.0, ci.rnd(64, seed=144) * 0.4
    out["naf_tail"] = (lambda dt: ci.naf_tail(gt, y, w3, b3, w4, b4, w5, b5, sca, beta, gn, bn, gam, dt), famn)
    for off in (-8.0, 0.0, 8.0, 32.0):                      # the SpatialGate of test_sgfn_statistics, on the fp32 image of the fp64 fc1 output
        xs = ci.rnd(77, 180, seed=500, scale=1.5) + 0.3
        gs, bs = ci.ln_params(180, 501)
        ws1, bs1 = ci.lin_params(720, 180, 503)
        bs1 = bs1.clone()
        bs1[360:] += off
        g2, bb2 = ci.ln_params(360, 505)
        wdd, bdd = ci.rnd(360, 1, 3, 3, seed=507, scale=0.3), ci.rnd(360, seed=508, scale=0.1)
        ys = ci.token_linear(xs, gs, bs, 1e-5, ws1, bs1, "gelu", F64)[0].float()
        out[f"spatial_gate off={off:g}"] = (lambda dt, ys=ys, g2=g2, bb2=bb2, wdd=wdd, bdd=bdd: ci.spatial_gate(ys, 7, 11, g2, bb2, wdd, bdd, dt).reshape(77, 360), ci.ALL)
    wq, bq = ci.lin_params(540, 180, 50)
    temp = ci.rnd(6, seed=52) * 0.2 + 1.0
    xc, famc = ci.ln_rows(77, 180, seed=4, skip=("offset_1000_1",))
    out["chan_qkv v"] = (lambda dt: ci.chan_qkv(xc, g, b, wq, bq, temp, 6, dt)[0], famc)
    xh, famh = ci.ln_rows(256, 180, seed=7, skip=("offset_1000_1",))
    table = ci.rnd(6, 31 * 31, seed=54, scale=0.5)
    out["hat_attn"] = (lambda dt: ci.hat_attn(xh.reshape(1, 16, 16, 180), g, b, wq, bq, table, 6, 30, (16, 16), (8, 8), dt), famh)
    out["chan_qkv matrix"] = (lambda dt: ci.chan_qkv(x, g, b, wq, bq, temp, 6, dt)[1], ci.ALL)
    return out


CHAINS = _chains()


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_fp32_stand_in_stays_close_to_fp64_on_every_family(name):
    fn, fam = CHAINS[name]
    ref, st = fn(F64), fn(F32)
    ref, st = (ref, st) if isinstance(ref, tuple) else ((ref,), (st,))
    for r, s in zip(ref, st):
        assert r.dtype == F64 and s.dtype == F32 and torch.isfinite(r).all() and torch.isfinite(s).all()
        err = ci.family_errors(s, r, fam)
        print(name, {k: f"{v:.1e}" for k, v in err.items()})
        assert max(err.values()) <= ci.STANDIN_CAP, err


def test_check_rejects_an_error_hidden_by_a_large_block():
    """Per-family normalisation: an error of 1e-2 in the control rows is far below 6e-5 of the huge block's magnitude."""
    x, fam = ci.ln_rows(77, 180, seed=8)
    ref = x.double()
    bad = x.clone()
    bad[fam["control"]] += 1e-2
    assert (bad.double() - ref).abs().max() <= 6e-5 * ref.abs().max()
    with pytest.raises(AssertionError):
        ci.check(bad, ref, x, fam, 6e-5, "mutant")
    ci.check(x, ref, x, fam, 6e-5, "identity")


@pytest.mark.parametrize("family", ci.ATTN_FAMILIES)
def test_attention_families_have_precision_independent_answers(family):
    heads, d, win, H, W = 6, 30, (16, 16), 32, 32
    qkv, info = ci.attn_qkv(family, H, W, heads, d, win, seed=60)
    shift = (8, 8) if family == "masked" else (0, 0)
    zero = torch.zeros(heads, 31 * 31)
    ref = ci.window_attention(qkv, zero, heads, d, win, shift, F64)
    assert torch.isfinite(ref).all()
    C = heads * d
    roll = torch.roll(qkv, shifts=(-shift[0], -shift[1]), dims=(1, 2))
    q, k, v = [ci.win_split(roll[..., i * C:(i + 1) * C], 16, 16).reshape(4, 256, heads, d) for i in range(3)]
    if family in ("uniform", "masked"):
        assert (q == 0).all()
        lab = ci.region_labels(H, W, 16, 16, 8, 8) if family == "masked" else torch.zeros(4, 256)
        same = (lab.unsqueeze(1) == lab.unsqueeze(2)).double()                       # (nwin, nq, nk)
        mean_v = torch.einsum("wqk,wkhd->wqhd", same / same.sum(-1, keepdim=True), v.double())
        got = ci.win_split(torch.roll(ref, shifts=(-shift[0], -shift[1]), dims=(1, 2)), 16, 16).reshape(4, 256, heads, d)
        assert (got - mean_v).abs().max() < 1e-12
        if family == "masked":
            assert (same.sum(-1) < 256).any(), "the mask removes nothing"
    else:
        logits = torch.einsum("wqhd,wkhd->whqk", q.double() * d ** -0.5, k.double())
        top2 = logits.topk(3, dim=-1).values
        if family == "onehot":
            assert (top2[..., 0] - top2[..., 1]).min() >= 40
        else:
            wi, hi = torch.meshgrid(torch.arange(4), torch.arange(heads), indexing="ij")
            assert torch.equal(k[wi, info["winner"], hi], k[wi, info["second"], hi])
            assert (top2[..., 0] == top2[..., 1]).all() and (top2[..., 0] - top2[..., 2]).min() >= 40
        exact = ci.attn_exact(family, q, k, v, info)
        got = ci.win_split(ref, 16, 16).reshape(4, 256, heads, d)
        assert (got - exact).abs().max() < 1e-12
        assert (ci.window_attention(qkv, zero, heads, d, win, shift, F32).double() - ref).abs().max() < 1e-5


@pytest.mark.parametrize("win", [(16, 16), (8, 32)])
@pytest.mark.parametrize("family", ci.ATTN_FAMILIES)
def test_projected_attention_families(family, win):
    """The families of win_attn_fused: after the fp64 projection q is exactly 0 (`uniform`, `masked`) or the winner leads by >= 40 and the
    tied keys are bit-identical in fp32 too; the answer is the projected v row of the winner(s)."""
    heads, d, H, W, C = 6, 30, 32, 32, 180
    x, w, b, info = ci.attn_proj_case(family, H, W, win, heads, d, seed=62)
    shift = (win[0] // 2, win[1] // 2) if family == "masked" else (0, 0)
    table = torch.zeros(heads, (2 * win[0] - 1) * (2 * win[1] - 1))
    ref, v = ci.proj_attention(x, w, b, table, heads, d, win, shift, F64)
    qkv = ci.linear(x.reshape(H * W, C), w, b, F64).reshape(1, H, W, 3 * C)
    n = win[0] * win[1]
    if family in ("uniform", "masked"):
        assert (qkv[..., :C] == 0).all() and (ci.linear(x.reshape(H * W, C), w, b, F32)[:, :C] == 0).all()
        lab = ci.region_labels(H, W, *win, *shift) if family == "masked" else torch.zeros(4, n)
        same = (lab.unsqueeze(1) == lab.unsqueeze(2)).double()
        vw = ci.win_split(torch.roll(v, shifts=(-shift[0], -shift[1]), dims=(1, 2)), *win)
        got = ci.win_split(torch.roll(ref, shifts=(-shift[0], -shift[1]), dims=(1, 2)), *win)
        assert (got - (same / same.sum(-1, keepdim=True)) @ vw).abs().max() < 1e-12
    else:
        q, k = [ci.win_split(qkv[..., i * C:(i + 1) * C], *win).reshape(4, n, heads, d) for i in range(2)]
        top = torch.einsum("wqhd,wkhd->whqk", q * d ** -0.5, k).topk(3, dim=-1).values
        lead = top[..., 0] - top[..., 1 if family == "onehot" else 2]
        assert lead.min() >= 40
        if family == "tie":
            k32 = ci.win_split(ci.linear(x.reshape(H * W, C), w, b, F32).reshape(1, H, W, 3 * C)[..., C:2 * C], *win).reshape(4, n, heads, d)
            wi, hi = torch.meshgrid(torch.arange(4), torch.arange(heads), indexing="ij")
            assert torch.equal(k32[wi, info["winner"], hi], k32[wi, info["second"], hi]) and (top[..., 0] == top[..., 1]).all()
        vw = ci.win_split(v, *win).reshape(4, n, heads, d)
        got = ci.win_split(ref, *win).reshape(4, n, heads, d)
        assert (got - ci.attn_exact(family, None, None, vw, info)).abs().max() < 1e-12


@pytest.mark.parametrize("family", ["uniform", "onehot", "tie"])
def test_ocab_families(family):
    """Overlapping key windows: every query window sees exactly its own winner(s), 40 above every other key AND above the zero-padded
    keys at logit 0; with q = 0 the answer is softmax(bias) over all 576 keys, padded ones (v = 0) included."""
    heads, d, ws, ows, H, W = 6, 30, 16, 24, 32, 32
    qkv, (q, k, v, info) = ci.ocab_qkv(family, H, W, heads, d, ws, seed=64)
    zero = torch.zeros((ws + ows - 1) ** 2, heads)
    ref = ci.ocab_attention(qkv, zero, heads, d, ws, ows, F64)
    got = ci.win_split(ref, ws, ws).reshape(4, ws * ws, heads, d)
    if family == "uniform":
        assert (q == 0).all()
        tot = ci.ocab_attention(torch.cat([qkv[..., :360], torch.ones(1, H, W, 180)], -1), zero, heads, d, ws, ows, F64)
        assert (tot - 400.0 / 576.0).abs().max() < 1e-12      # every window of a 32 x 32 image is a corner: 20 x 20 real keys of 24 x 24
    else:
        C = heads * d
        kv = torch.nn.functional.unfold(qkv[..., C:2 * C].permute(0, 3, 1, 2).double(), kernel_size=ows, stride=ws, padding=4)
        kh = kv.reshape(1, C, ows * ows, 4).permute(0, 3, 2, 1).reshape(4, ows * ows, heads, d)
        top = torch.einsum("wqhd,wkhd->whqk", q.double() * d ** -0.5, kh).topk(3, dim=-1).values
        assert (top[..., 0] - top[..., 1 if family == "onehot" else 2]).min() >= 40 and top[..., 0].min() >= 40
        assert (got - ci.attn_exact(family, q, k, v, info)).abs().max() < 1e-12


def test_one_pass_statistics_miss_the_bar_and_two_pass_forms_meet_it():
    """The emulation behind the SGFN statistics fix, n = 360 values per row: var = ssq / n - mean^2 from fp32 running sums is over the
    bar of test_conditioning_gpu.py on every offset family (and on GELU outputs with a shifted bias); two-pass sums in another
    order and the kernel's grouped pairwise form are within it."""
    x, fam = ci.ln_rows(109, 360, seed=9)
    rows = {n: x[fam[n]] for n in ci.OFFSET_FAMILIES}
    for off in (-8.0, 0.0, 8.0, 32.0):
        rows[f"gelu({off:+g})"] = ci.gelu(ci.rnd(77, 360, seed=11) + off).float()
    for name, v in rows.items():
        mr, rr, mean_bar, rstd_bar = ci.stats_bars(v)
        res = {}
        for form, fn in (("one-pass", ci.stats_one_pass_fp32), ("two-pass", ci.stats_two_pass_seq_fp32), ("grouped", ci.stats_grouped_fp32)):
            m, r = fn(v)
            res[form] = (((m.double() - mr).abs() / mean_bar).max().item(), ((r.double() - rr).abs() / rr).max().item())
        print(name, f"rstd bar {rstd_bar:.1e}", {k: f"{a[1]:.1e}" for k, a in res.items()}, "mean err / bar", {k: f"{a[0]:.2f}" for k, a in res.items()})
        if name not in ("gelu(-8)", "gelu(+0)"):                      # mean / std about 0 and 0.5: every form is fine there
            assert res["one-pass"][1] > rstd_bar, (name, res, rstd_bar)
        for form in ("two-pass", "grouped"):
            assert res[form][1] <= rstd_bar, (name, form, res, rstd_bar)
        assert res["grouped"][0] <= 1.0, (name, res)             # the kernel's form also meets the bar on the mean
