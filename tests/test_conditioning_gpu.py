"""The fp32-grade kernels on ill-conditioned rows (run with -m gpu on the MI355X box).

Every other op-level test feeds zero-mean, unit-scale randn rows and compares one max-abs error with the global max|ref|.  Here the
inputs are the families of tests/golden/cond_inputs.py -- rows with a DC offset, near-constant and constant rows, a massive activation,
tiny and huge rows; attention inputs with precision-independent answers; activation arguments far out in the tails; eps guards hit
exactly -- in 'bf16x3', the parity-grade mode, against fp64 chains.  The rule (cond_inputs.check): errors per family, normalised by
that family's max(1, max|ref|); allowance = the op's bar in tests/test_ops_gpu.py + 4 x the error of the same chain in torch fp32 on the
CPU on these very tensors.  tests/test_cond_inputs_cpu.py shows that every family used here is inside what fp32 arithmetic can do.

Families left out, and why (cond_inputs.STANDIN_CAP = 1e-4 is the line): `lowvar` at m = 5 everywhere (a bare fp32 LayerNorm is 1e-4 to
2.8e-4 from fp64 on it); `offset (1000, 1)` for chan_qkv_attn (stand-in 1.5e-4 on v) and for win_attn_fused (1.0e-4: one window's
softmax spreads that block's error over every row).
Two ops exist for the plain-bf16 mode only and are run in it, at their plain-bf16 bars: ocab_attn on the attention families (precision-
independent answers, so the bar of tests/test_ops_gpu.py holds as it stands) and naf_tail on the LayerNorm families."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import cond_inputs as ci  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
GEMM_TOL = {"f32": 2e-5, "bf16x3": 6e-5, "bf16": 2e-2}      # tests/test_ops_gpu.py


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isr2_amd import lib, ops
    lib.load()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    old = ops.gemm_mode()
    ops.set_gemm_mode("bf16x3")
    yield torch.device("cuda:0")
    ops.set_gemm_mode(old)


def padded(t, dev):
    """rows [M, C] -> a device view with the row pitch rounded up to 32 floats (what ops.empty_rows produces)."""
    C = t.shape[-1]
    buf = torch.empty(tuple(t.shape[:-1]) + ((C + 31) // 32 * 32,), device=dev)[..., :C]
    buf.copy_(t)
    return buf


def to(dev, *ts):
    return [t.to(dev).contiguous() for t in ts]


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm-bearing ops
@pytest.mark.parametrize("C,eps,M", [(180, 1e-5, 77), (64, 1e-6, 77), (1024, 1e-6, 109)])
def test_layernorm(dev, C, eps, M):
    from isr2_amd import ops
    x, fam = ci.ln_rows(M, C, seed=2)
    g, b = ci.ln_params(C, 10)
    ref, st = ci.layernorm(x, g, b, eps, F64), ci.layernorm(x, g, b, eps, F32)
    xd, gd, bd = to(dev, x, g, b)
    out = ops.layernorm(xd, gd, bd, eps)
    ci.check(out, ref, st, fam, 1e-5, f"layernorm C={C}")
    c3 = fam["const_3"]
    assert torch.equal(out[c3].cpu(), b.expand(c3.stop - c3.start, C)), "constant rows: the output must be beta bit for bit"
    wide = torch.zeros(M, 2 * C + 8, device=dev)                             # the strided-slice form
    wide[:, C + 8:] = xd
    out2 = ops.layernorm(wide[:, C + 8:], gd, bd, eps)
    ci.check(out2, ref, st, fam, 1e-5, f"layernorm slice C={C}")
    assert torch.equal(out2[c3].cpu(), b.expand(c3.stop - c3.start, C))


@pytest.mark.parametrize("K,N,eps", [(180, 180, 1e-5), (64, 128, 1e-6)])
def test_token_linear(dev, K, N, eps):
    from isr2_amd import ops
    from isr2_amd.prep import pack_token_linear
    M = 77
    x, fam = ci.ln_rows(M, K, seed=3)
    g, b = ci.ln_params(K, 20)
    w, bias = ci.lin_params(N, K, 22)
    (ref, xn_ref), (st, xn_st) = ci.token_linear(x, g, b, eps, w, bias, "gelu", F64), ci.token_linear(x, g, b, eps, w, bias, "gelu", F32)
    xd = padded(x, dev)
    gd, bd, wd, biasd = to(dev, g, b, w, bias)
    out, xn = ops.token_linear(xd, pack_token_linear(wd, biasd), gamma=gd, beta=bd, eps=eps, act="gelu", want_xn=True)
    ci.check(out, ref, st, fam, GEMM_TOL["bf16x3"], f"token_linear K={K}")
    ci.check(xn, xn_ref, xn_st, fam, 1e-5, f"token_linear xn K={K}")
    c3 = fam["const_3"]
    assert torch.equal(xn[c3].cpu(), b.expand(c3.stop - c3.start, K)), "constant rows: xn must be beta bit for bit"
    out2 = ops.token_linear(xd, pack_token_linear(wd, biasd), gamma=gd, beta=bd, eps=eps, act="gelu")
    assert torch.equal(out, out2)


def _mlp_case():
    x, fam = ci.ln_rows(77, 180, seed=4)
    g, b = ci.ln_params(180, 30)
    w1, b1 = ci.lin_params(360, 180, 32)
    w2, b2 = ci.lin_params(180, 360, 34)
    return x, fam, g, b, w1, b1, w2, b2


def test_token_mlp(dev):
    from isr2_amd import ops
    from isr2_amd.prep import pack_token_mlp
    x, fam, g, b, w1, b1, w2, b2 = _mlp_case()
    ref, st = ci.token_mlp(x, g, b, w1, b1, w2, b2, F64), ci.token_mlp(x, g, b, w1, b1, w2, b2, F32)
    out = ops.token_mlp(padded(x, dev), *to(dev, g, b), pack_token_mlp(*to(dev, w1, b1, w2, b2)))
    ci.check(out, ref, st, fam, 6e-5, "token_mlp")


def test_token_projmlp(dev):
    """norm2 is taken from the accumulators (x1 = x + proj(att)), so the offset sits on x."""
    from isr2_amd import ops
    from isr2_amd.prep import pack_token_projmlp
    x, fam, g, b, w1, b1, w2, b2 = _mlp_case()
    att = ci.rnd(77, 180, seed=36)
    wp, bp = ci.lin_params(180, 180, 37)
    ref, st = [ci.token_projmlp(att, x, wp, bp, w1, b1, w2, b2, g, b, dt) for dt in (F64, F32)]
    out = ops.token_projmlp(padded(att, dev), padded(x, dev), pack_token_projmlp(*to(dev, wp, bp, w1, b1, w2, b2)), *to(dev, g, b))
    ci.check(out, ref, st, fam, GEMM_TOL["bf16x3"], "token_projmlp")


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_win_attn_fused_hat(dev, mode):
    """HAT form, one 16x16 window, shift 8, gamma / beta: the normalised rows and the attention output.  No `offset (1000, 1)`: see the
    module docstring.  'bf16': the plain-bf16 kernel (another LayerNorm text) writes the same fp32 normalised rows, held to the same
    2e-6; its attention output has no fp32-grade bar and is only required to be finite.
    Before the corrected two-pass statistics of both kernels the `const 0.1` rows came out 8.8e-6 from beta (allowance 2e-6)."""
    from isr2_amd import ops
    from isr2_amd.prep import pack_win_attn, pack_win_rel
    heads, d, ws, C, H, W = 6, 30, 16, 180, 16, 16
    x, fam = ci.ln_rows(H * W, C, seed=7, skip=("offset_1000_1",))
    g, b = ci.ln_params(C, 30)
    wq, bq = ci.lin_params(3 * C, C, 50)
    table = ci.rnd(heads, (2 * ws - 1) ** 2, seed=54, scale=0.5)
    (xn_ref, ref), (xn_st, st) = [ci.hat_attn(x.reshape(1, H, W, C), g, b, wq, bq, table, heads, d, (ws, ws), (8, 8), dt) for dt in (F64, F32)]
    gd, bd, wqd, bqd, td = to(dev, g, b, wq, bq, table)
    out = ops.empty_rows((1, H, W, C), dev)
    out.zero_()
    old = ops.gemm_mode()
    ops.set_gemm_mode(mode)
    try:
        _, xn = ops.win_attn_fused(padded(x.reshape(1, H, W, C), dev), out, pack_win_attn(wqd, bqd, heads, d, d ** -0.5),
                                   pack_win_rel(td, ws, ws), gamma=gd, beta=bd, H=H, W=W, Hp=H, Wp=W, win=(ws, ws), shift=(8, 8),
                                   use_mask=True, want_xn=True)
    finally:
        ops.set_gemm_mode(old)
    ci.check(xn.reshape(H * W, C), xn_ref, xn_st, fam, 2e-6, f"win_attn_fused xn {mode}")
    c3 = fam["const_3"]
    assert torch.equal(xn.reshape(H * W, C)[c3].cpu(), b.expand(c3.stop - c3.start, C)), "constant rows: xn must be beta bit for bit"
    if mode == "bf16x3":
        ci.check(out.reshape(H * W, C), ref, st, fam, GEMM_TOL["bf16x3"], "win_attn_fused")
    else:
        assert torch.isfinite(out).all()


def test_chan_qkv_attn(dev):
    """The v side output per family and the channel-attention matrix (one block: it sums over every row).  No `offset (1000, 1)`: see
    the module docstring."""
    from isr2_amd import ops
    from isr2_amd.prep import pack_chan_qkv
    C, heads, M = 180, 6, 77
    x, fam = ci.ln_rows(M, C, seed=4, skip=("offset_1000_1",))
    g, b = ci.ln_params(C, 30)
    wq, bq = ci.lin_params(3 * C, C, 50)
    temp = ci.rnd(heads, seed=52) * 0.2 + 1.0
    (v_ref, a_ref), (v_st, a_st) = [ci.chan_qkv(x, g, b, wq, bq, temp, heads, dt) for dt in (F64, F32)]
    gd, bd, wqd, bqd, td = to(dev, g, b, wq, bq, temp)
    v, wbd = ops.chan_qkv_attn(padded(x, dev), pack_chan_qkv(wqd, bqd), gd, bd, td)
    ci.check(v, v_ref, v_st, fam, GEMM_TOL["bf16x3"], "chan_qkv_attn v")
    ci.check(wbd, a_ref, a_st, ci.ALL, 2e-5, "chan_qkv_attn matrix")


def _naf_case(M):
    y, fam = ci.ln_rows(M, 64, seed=5 if M == 77 else 6)
    g, b = ci.ln_params(64, 40)
    w4, b4 = ci.lin_params(128, 64, 42)
    return y, fam, g, b, w4, b4


def test_naf_front(dev):
    """C = 64, 9 x 17 pixels: the families are runs of pixels, the depth-wise taps reach across them."""
    from isr2_amd import ops
    from isr2_amd.prep import pack_token_linear, pack_dw
    H, W, C = 9, 17, 64
    x, fam, g, b, w1, b1 = _naf_case(H * W)
    wd, bd = ci.rnd(2 * C, 1, 3, 3, seed=47, scale=0.3), ci.rnd(2 * C, seed=48, scale=0.1)
    (ref, p_ref), (st, p_st) = [ci.naf_front(x.reshape(H, W, C), g, b, w1, b1, wd, bd, dt) for dt in (F64, F32)]
    gd, bdev, w1d, b1d, wdd, bdd = to(dev, g, b, w1, b1, wd, bd)
    got, pooled = ops.naf_front(x.reshape(1, H, W, C).to(dev).contiguous(), pack_token_linear(w1d, b1d), gd, bdev, pack_dw(wdd), bdd)
    ci.check(got.reshape(H * W, C), ref.reshape(H * W, C), st.reshape(H * W, C), fam, 2 * GEMM_TOL["bf16x3"], "naf_front")
    ci.check(pooled.reshape(1, C), p_ref.reshape(1, C), p_st.reshape(1, C), ci.ALL, 2 * GEMM_TOL["bf16x3"], "naf_front pool")


def test_naf_ffn(dev):
    from isr2_amd import ops
    from isr2_amd.prep import pack_naf_ffn
    y, fam, g, b, w4, b4 = _naf_case(77)
    w5, b5 = ci.lin_params(64, 64, 44)
    gam = ci.rnd(64, seed=46, scale=0.3)
    ref, st = [ci.naf_ffn(y, g, b, w4, b4, w5, b5, gam, dt) for dt in (F64, F32)]
    out = ops.naf_ffn(y.to(dev), pack_naf_ffn(*to(dev, w4, b4, w5, b5)), *to(dev, g, b, gam))
    ci.check(out, ref, st, fam, 6e-5, "naf_ffn")


def test_naf_tail(dev):
    """C = 64, M = 77.  The kernel exists for the plain-bf16 mode only, so it runs in it: the families sit on x (the LayerNorm operand is
    y = x + beta * conv3(g * sca)), per-family errors, allowance = its plain-bf16 bar (3e-2, tests/test_naf_tail_gpu.py) + 4 x the fp32
    stand-in's error."""
    from isr2_amd import ops
    from isr2_amd.prep import pack_naf_tail
    C, M = 64, 77
    x, fam, ln_g, ln_b, w4, b4 = _naf_case(M)
    g = ci.rnd(M, C, seed=140)
    w3, b3 = ci.lin_params(C, C, 141)
    w5, b5 = ci.lin_params(C, C, 44)
    sca, beta, gamma = ci.rnd(C, seed=143) * 0.3 + 1.0, ci.rnd(C, seed=144) * 0.4, ci.rnd(C, seed=46, scale=0.3)
    ref, st = [ci.naf_tail(g, x, w3, b3, w4, b4, w5, b5, sca, beta, ln_g, ln_b, gamma, dt) for dt in (F64, F32)]
    old = ops.gemm_mode()
    ops.set_gemm_mode("bf16")
    try:
        out = ops.naf_tail(g.to(dev), x.to(dev), pack_naf_tail(*to(dev, w3, b3, w4, b4, w5, b5)), *to(dev, sca, beta, ln_g, ln_b, gamma))
    finally:
        ops.set_gemm_mode(old)
    ci.check(out, ref, st, fam, 3e-2, "naf_tail (plain bf16)")


# ---------------------------------------------------------------------------------------------------------------
# SGFN statistics: the LayerNorm (mean, rstd) side output of ff_token_linear
def _sgfn_case(dev, off):
    C, Hd, H, W = 180, 720, 7, 11
    c2 = Hd // 2
    x = ci.rnd(H * W, C, seed=500, scale=1.5) + 0.3
    g, b = ci.ln_params(C, 501)
    w1, b1 = ci.lin_params(Hd, C, 503)
    b1 = b1.clone()
    b1[c2:] += off
    g2, bb2 = ci.ln_params(c2, 505)
    wd, bd = ci.rnd(c2, 1, 3, 3, seed=507, scale=0.3), ci.rnd(c2, seed=508, scale=0.1)
    return C, Hd, H, W, c2, x, g, b, w1, b1, g2, bb2, wd, bd


@pytest.mark.parametrize("off", [-8.0, 0.0, 8.0, 32.0])
def test_sgfn_statistics(dev, off):
    """fc1 + GELU with the statistics of the activated upper half, C = 180, Hd = 720, M = 77; `off` on the upper half's bias gives that
    half a mean / std of about 0 (variance far below eps), 0.5, 8 and 32.  The reference statistics are fp64 of the kernel's OWN
    output, so contraction error does not enter; the bars are 4 x the two-pass fp32 stand-in's error on the same values (the mean with
    a floor of 2^-22 max(1, |mean|)).  Then the consumer, ff_dwconv3x3_ln at 7 x 11, against the fp64 SpatialGate of the same y.
    Measured on the MI355X, relative rstd error (bar): the one-pass kernel this replaced 6.8e-8 (2.7e-7), 2.8e-7 (5.7e-7), 2.3e-5
    (4.5e-7: failed), 4.0e-4 (4.0e-7: failed); this kernel 6.8e-8, 1.8e-7, 1.4e-7, 1.8e-7."""
    from isr2_amd import ops
    from isr2_amd.prep import pack_token_linear, pack_dw
    C, Hd, H, W, c2, x, g, b, w1, b1, g2, bb2, wd, bd = _sgfn_case(dev, off)
    M = H * W
    xd = padded(x.reshape(1, H, W, C), dev)
    gd, bdev, w1d, b1d, g2d, bb2d, wdd, bdd = to(dev, g, b, w1, b1, g2, bb2, wd, bd)
    y, stats = ops.token_linear(xd, pack_token_linear(w1d, b1d), gamma=gd, beta=bdev, act="gelu", stats_range=(c2, Hd))
    yc = y.reshape(M, Hd).cpu()
    assert torch.isfinite(yc).all() and torch.isfinite(stats).all()
    y_ref = ci.token_linear(x, g, b, 1e-5, w1, b1, "gelu", F64)[0]
    assert (yc.double() - y_ref).abs().max() <= GEMM_TOL["bf16x3"] * y_ref.abs().max().clamp_min(1.0)
    v = yc[:, c2:]
    mr, rr, mean_bar, rstd_bar = ci.stats_bars(v)
    sc = stats.cpu().double()
    mean_err, rstd_err = (sc[:, 0] - mr).abs(), (sc[:, 1] - rr).abs() / rr
    ratio = (mr.abs() / v.double().std(-1, unbiased=False).clamp_min(1e-30)).median().item()
    print(f"sgfn stats off={off:g}: mean/std {ratio:.2g}, mean err {mean_err.max().item():.2e} (bar {mean_bar.min().item():.2e}), "
          f"rstd rel err {rstd_err.max().item():.2e} (bar {rstd_bar:.2e})")
    assert (mean_err <= mean_bar).all(), f"mean: {mean_err.max().item():.3e} over {mean_bar.min().item():.3e}"
    assert rstd_err.max().item() <= rstd_bar, f"rstd: relative error {rstd_err.max().item():.3e} over {rstd_bar:.3e}"
    z = ops.dwconv3x3_ln(y[..., c2:], pack_dw(wdd), bdd, stats, g2d, bb2d, mul_in=y[..., :c2])
    ref, st = [ci.spatial_gate(yc, H, W, g2, bb2, wd, bd, dt).reshape(M, c2) for dt in (F64, F32)]
    ci.check(z.reshape(M, c2), ref, st, ci.ALL, 1e-4, f"SpatialGate on load off={off:g}")


# ---------------------------------------------------------------------------------------------------------------
# attention on inputs with precision-independent answers
def _attn_close(out, ref, tol, name):
    out = out.detach().cpu().double()
    assert torch.isfinite(out).all(), f"{name}: non-finite output"
    err, mag = (out - ref).abs().max().item(), max(1.0, ref.abs().max().item())
    print(f"{name}: max|d| = {err:.2e} (bar {tol * mag:.2e})")
    assert err <= tol * mag, f"{name}: max|d|={err:.3e} ref={mag:.3e}"


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
@pytest.mark.parametrize("family", ci.ATTN_FAMILIES)
def test_window_attn(dev, mode, family):
    """32 x 32, 16 x 16 windows, 6 heads of 30.  `uniform` carries a random relative-position bias (the logits are that bias alone), the
    others a zero one; `masked` is shifted by 8."""
    from isr2_amd import ops
    heads, d, ws, C, H, W = 6, 30, 16, 180, 32, 32
    qkv, info = ci.attn_qkv(family, H, W, heads, d, (ws, ws), seed=60)
    table = ci.rnd(heads, (2 * ws - 1) ** 2, seed=61, scale=0.5) if family == "uniform" else torch.zeros(heads, (2 * ws - 1) ** 2)
    shift = (8, 8) if family == "masked" else (0, 0)
    ref = ci.window_attention(qkv, table, heads, d, (ws, ws), shift, F64)
    if family in ("onehot", "tie"):                                     # the reference IS the exact answer
        q, k, v = [ci.win_split(qkv[..., i * C:(i + 1) * C], ws, ws).reshape(4, ws * ws, heads, d) for i in range(3)]
        exact = ci.win_merge(ci.attn_exact(family, q, k, v, info).reshape(4, ws * ws, C), ws, ws, H, W)
        assert (ref - exact).abs().max() < 1e-12
    biasT = table[:, ci.rel_index(ws, ws)].transpose(1, 2).contiguous().to(dev)
    out = torch.zeros(1, H, W, C, device=dev)
    old = ops.gemm_mode()
    ops.set_gemm_mode(mode)
    try:
        ops.window_attn(qkv.to(dev), out, biasT, q_off=0, k_off=C, v_off=2 * C, o_off=0, H=H, W=W, Hp=H, Wp=W, win=(ws, ws), kwin=(ws, ws),
                        shift=shift, use_mask=family == "masked", heads=heads, d=d, scale=d ** -0.5)
    finally:
        ops.set_gemm_mode(old)
    _attn_close(out, ref, GEMM_TOL[mode], f"window_attn {mode} {family}")


@pytest.mark.parametrize("form", ["hat", "dat"])
@pytest.mark.parametrize("family", ci.ATTN_FAMILIES)
def test_win_attn_fused_attention_families(dev, form, family):
    """The attention families through the fused kernel's own qkv projection (cond_inputs.attn_proj_case; no LayerNorm), 32 x 32, bf16x3:
    HAT (16 x 16 windows, all six heads, shift 8 for `masked`) and one DAT branch (8 x 32 windows, heads 0-2 of the packed six, zero
    tokens beyond (H, W), shift (4, 16) for `masked`).  `uniform` carries a random bias table.  The exact answer of `onehot` / `tie` is
    the fp64-projected v row of the winner(s)."""
    from isr2_amd import ops
    from isr2_amd.prep import pack_win_attn, pack_win_rel
    heads, d, C, H, W = 6, 30, 180, 32, 32
    win, nh = ((16, 16), 6) if form == "hat" else ((8, 32), 3)
    shift = (win[0] // 2, win[1] // 2) if family == "masked" else (0, 0)
    x, wq, bq, info = ci.attn_proj_case(family, H, W, win, heads, d, seed=62)
    nrel = (2 * win[0] - 1) * (2 * win[1] - 1)
    table = torch.zeros(heads, nrel)
    if family == "uniform":
        table[:nh] = ci.rnd(nh, nrel, seed=63, scale=0.5)
    ref, v64 = ci.proj_attention(x, wq, bq, table, heads, d, win, shift, F64)
    if family in ("onehot", "tie"):
        n = win[0] * win[1]
        vw = ci.win_split(v64, *win).reshape(-1, n, heads, d)
        exact = ci.win_merge(ci.attn_exact(family, None, None, vw, info).reshape(-1, n, C), *win, H, W)
        assert (ref - exact).abs().max() < 1e-12
    wqd, bqd, td = to(dev, wq, bq, table)
    out = ops.empty_rows((1, H, W, C), dev)
    out.zero_()
    kw = dict(head0=0, nheads=3, zero_pad=True) if form == "dat" else {}
    ops.win_attn_fused(padded(x, dev), out, pack_win_attn(wqd, bqd, heads, d, d ** -0.5), pack_win_rel(td, *win), gamma=None, beta=None,
                       H=H, W=W, Hp=H, Wp=W, win=win, shift=shift, use_mask=family == "masked", **kw)
    _attn_close(out[..., :nh * d], ref[..., :nh * d], GEMM_TOL["bf16x3"], f"win_attn_fused {form} {family}")


@pytest.mark.parametrize("family", ["uniform", "onehot", "tie"])
def test_ocab_attn(dev, family):
    """HAT OCAB at 32 x 32 (16 x 16 query windows, 24 x 24 zero-padded key windows).  The kernel exists for the plain-bf16 mode only, so
    it runs in it, at its bar there (GEMM_TOL["bf16"]): the answers do not depend on the precision of the logits.  The zero-padded keys
    sit at logit 0 (plus bias) and carry v = 0: `uniform` includes them in the denominator, and the winner of `onehot` / `tie` is at
    logit >= 44, 40 above them as well.  No mask exists here, so no `masked`."""
    from isr2_amd import ops
    from isr2_amd.prep import pack_rel_overlap
    heads, d, ws, ows, C, H, W = 6, 30, 16, 24, 180, 32, 32
    qkv, (q, k, v, info) = ci.ocab_qkv(family, H, W, heads, d, ws, seed=64)
    n = (ws + ows - 1) ** 2
    table = ci.rnd(n, heads, seed=65, scale=0.5) if family == "uniform" else torch.zeros(n, heads)
    ref = ci.ocab_attention(qkv, table, heads, d, ws, ows, F64)
    if family != "uniform":
        exact = ci.win_merge(ci.attn_exact(family, q, k, v, info).reshape(-1, ws * ws, C), ws, ws, H, W)
        assert (ref - exact).abs().max() < 1e-12
    out = ops.empty_rows((1, H, W, C), dev)
    out.zero_()
    old = ops.gemm_mode()
    ops.set_gemm_mode("bf16")
    try:
        ops.ocab_attn(qkv.to(dev), out, pack_rel_overlap(table.to(dev), ws, ows), q_off=0, k_off=C, v_off=2 * C, H=H, W=W, heads=heads, d=d,
                      ws=ws, ows=ows, scale=d ** -0.5)
    finally:
        ops.set_gemm_mode(old)
    _attn_close(out, ref, GEMM_TOL["bf16"], f"ocab_attn {family}")


@pytest.mark.parametrize("family", ["uniform", "onehot", "tie"])
def test_band_mha_core(dev, family):
    """P = 64 pixels, 9 bands, 4 heads of 16 (no mask exists here, so no `masked`)."""
    from isr2_amd import ops
    P, nb, heads, E = 64, 9, 4, 64
    q, k, v, info = ci.attn_tokens(family, P, nb, heads, E // heads, seed=70)
    qkv = torch.cat([t.reshape(P * nb, E) for t in (q, k, v)], dim=-1).contiguous()
    ref = ci.band_mha(qkv, P, nb, heads, F64)
    if family != "uniform":
        assert (ref - ci.attn_exact(family, q, k, v, info).reshape(P * nb, E)).abs().max() < 1e-12
    else:
        assert (ref.reshape(P, nb, E) - v.double().reshape(P, nb, E).mean(1, keepdim=True)).abs().max() < 1e-12
    _attn_close(ops.band_mha_core(qkv.to(dev), P, nb, heads), ref, 1e-5, f"band_mha_core {family}")


# ---------------------------------------------------------------------------------------------------------------
# activation tails and eps guards
def _ulp32(t):
    return torch.from_numpy(np.spacing(np.abs(t.detach().cpu().float().numpy())).astype(np.float64))


def test_gelu_tail(dev):
    """ff_gelu_fast pinned to the Abramowitz-Stegun bound its header cites (|erf error| <= 1.5e-7): a grid passes through a centre-tap-only
    depth-wise 3x3 exactly (weight 1 at the centre, 0 elsewhere, no bias), 4096 points on [-12, 12] plus +-1e4 and +-1e20."""
    from isr2_amd import ops
    from isr2_amd.prep import pack_dw
    H, W, C = 10, 41, 10
    v = torch.cat([torch.linspace(-12, 12, 4096, dtype=F64).float(), torch.tensor([1e4, -1e4, 1e20, -1e20])])
    assert v.numel() == H * W * C
    g = torch.Generator(device="cpu").manual_seed(80)
    v = v[torch.randperm(v.numel(), generator=g)]                           # the extremes land among ordinary neighbours
    w = torch.zeros(C, 1, 3, 3)
    w[:, 0, 1, 1] = 1.0
    out = ops.dwconv2d(v.reshape(1, H, W, C).to(dev), pack_dw(w.to(dev)), None, act="gelu").reshape(-1).cpu()
    assert not torch.isnan(out).any() and torch.isfinite(out).all()
    ref = ci.gelu(v.double())
    err, bound = (out.double() - ref).abs(), 0.5 * v.double().abs() * 1.5e-7 + 4 * _ulp32(out)
    worst = (err / bound).argmax().item()
    print(f"gelu tail: worst err/bound {(err / bound).max().item():.3f} at v = {v[worst].item():.6g} (err {err[worst].item():.2e})")
    assert (err <= bound).all(), f"v = {v[worst].item()}: |out - gelu| = {err[worst].item():.3e} over {bound[worst].item():.3e}"


SIG_ARGS = [-1e4, -104.0, -88.0, -30.0, 30.0, 88.0, 104.0, 1e4]


def _sigmoid_checks(out, name):
    out = out.reshape(-1).cpu()
    ref = torch.sigmoid(torch.tensor(SIG_ARGS, dtype=F64)).float()
    assert torch.isfinite(out).all(), f"{name}: {out}"
    assert (out[1:] >= out[:-1]).all(), f"{name}: not monotone: {out}"
    ulps = (out.double() - ref.double()).abs() / _ulp32(ref)
    print(f"{name}: {out.tolist()} ulps {ulps.tolist()}")
    assert (ulps <= 2).all(), f"{name}: {out.tolist()} against {ref.tolist()} ({ulps.tolist()} ulp)"


def test_sigmoid_tail(dev):
    """The sigmoid epilogue at +-30, +-88, +-104, +-1e4 through ops.affine and ops.pixel_mlp: finite, monotone, within 2 ulp of the
    fp64 value rounded to fp32."""
    from isr2_amd import ops
    C = 4
    a = torch.tensor(SIG_ARGS).reshape(-1, 1).expand(-1, C).contiguous().to(dev)
    out = ops.affine(a, torch.ones(C, device=dev), torch.zeros(C, device=dev), "sigmoid")
    for c in range(C):
        _sigmoid_checks(out[:, c], "affine sigmoid")
    W1 = torch.zeros(1, C, device=dev)
    W1[0, 0] = 1.0
    out = ops.pixel_mlp(a, W1, torch.zeros(1, device=dev), None, torch.ones(1, 1, device=dev), 0.0, "sigmoid")
    _sigmoid_checks(out, "pixel_mlp sigmoid")


def test_freq_guidance_on_a_zero_pixel(dev):
    from isr2_amd import ops
    b3 = ci.rnd(1, 5, 7, 9, seed=90)
    b3[0, 2, 3] = 0.0
    b3[0, 0, 0] = 0.0
    m = b3.double().reshape(1, 5, 7, 3, 3).abs().mean(-1)
    ref = torch.stack([m[..., 2], m[..., 1], m[..., 0]], -1) / (m.sum(-1, keepdim=True) + 1e-8)
    out = ops.freq_guidance(b3.to(dev)).cpu()
    assert torch.isfinite(out).all() and (out[0, 2, 3] == 0).all() and (out[0, 0, 0] == 0).all()
    assert (out.double() - ref).abs().max().item() <= 1e-6 * max(1.0, ref.abs().max().item())


def test_fuse_blend_with_all_gates_zero(dev):
    """All three gates exactly 0 on a 3 x 3 block of LR pixels: the HR pixels inside it see a gate sum of exactly 0 -> 0 / (0 + 1e-8)."""
    from isr2_amd import ops
    Hl, Wl = 6, 7
    Hh, Wh = 4 * Hl, 4 * Wl
    E, hier = ci.rnd(1, Hh, Wh, 9, seed=91).abs(), ci.rnd(1, Hh, Wh, 3, seed=92).abs()
    guide = torch.softmax(ci.rnd(1, Hl, Wl, 3, seed=93), -1)
    gates = torch.sigmoid(ci.rnd(1, Hl, Wl, 3, seed=94))
    gates[0, 1:4, 2:5] = 0.0
    dif = torch.sigmoid(ci.rnd(1, Hl, Wl, 1, seed=95))
    out = ops.fuse_blend(*to(dev, E, hier, guide, gates, dif)).cpu()

    def up(t):
        return F.interpolate(t.double().permute(0, 3, 1, 2), size=(Hh, Wh), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)

    g, gt, df = up(guide), up(gates), up(dif)
    assert (gt.sum(-1) == 0).any(), "no HR pixel with an all-zero gate sum"
    ex = [E[..., 0:3].double(), E[..., 3:6].double(), E[..., 6:9].double()]
    f0 = hier.double() * 0.7 + 0.3 * sum(e * g[..., i:i + 1] for i, e in enumerate(ex))
    dyn = sum(e * gt[..., i:i + 1] for i, e in enumerate(ex)) / (gt.sum(-1, keepdim=True) + 1e-8)
    ref = f0 * (1 - 0.3 * df) + dyn * (0.3 * df)
    assert torch.isfinite(out).all()
    assert (out.double() - ref).abs().max().item() <= 2e-6 * max(1.0, ref.abs().max().item())


def test_dynamic_gates_on_and_far_from_the_threshold(dev):
    """dif = 0 makes the threshold 0.7f exactly; a gate ON it is sigmoid(0) = 0.5, gates 1e3 away saturate to 0 and 1."""
    from isr2_amd import ops
    th = float(torch.tensor(0.7, dtype=F32))
    pix = [(th, th - 1e3, th + 1e3), (th, th, th), (th, th - 1e3, th - 1e3), (th + 1e3, th + 1e3, th - 1e3), (th - 1e3, th - 1e3, th - 1e3)]
    g = torch.tensor(pix, dtype=F32).reshape(1, 1, len(pix), 3)
    d = torch.zeros(1, 1, len(pix), 1)
    out = ops.dynamic_gates(g.to(dev), d.to(dev)).cpu()
    s = torch.sigmoid(10.0 * (g.double() - (0.7 - 0.4 * d.double())))
    mx = s.max(dim=-1, keepdim=True).values
    ref = torch.maximum(s, (s >= mx * 0.99).double() * 0.9)
    assert torch.isfinite(out).all()
    assert (out.double() - ref).abs().max().item() <= 1e-5, (out, ref)
