"""The plain-bf16 ('bf16', one MFMA term) and 'bf16x2' (exact activations x bf16 weights, two terms) kernels against an
OPERAND-ROUNDED fp64 reference (tests/golden/lowprec_ref.py), on the MI355X.

The bf16 MFMA multiplies bf16 operands exactly and accumulates in fp32.  The reference therefore rounds the operands the way the
staging path does -- A = bf16_rne(x) (kmul applied first, in fp32) or hi + bf16_rne(x - hi); W = bf16_rne(w) -- multiplies in
fp64, applies the epilogue in fp64, and the kernel is held to the project's fp32-accumulation bound, 2e-5 of max(1, max|ref|),
instead of the 1.5e-2 .. 3e-2 a comparison with an fp32 reference needs in these modes.  Rounding the operands alone moves a result by
about 2.5e-3 of max|ref|; truncation instead of round-to-nearest-even, a scale applied after the rounding or a double rounding are of
that size and are what these tests exist to see.  Activations: the implicit GEMM and the LDS-resident 3x3 kernel use the erf GELU
(ff_gelu_fast, |error| <= 1.5e-7), token_linear in plain bf16 the tanh form (ff_gelu_sig2).  bf16 output rows are held to half a bf16
ulp on top of the fp32 bound.  Every implicit-GEMM and halo case also asserts the route it took.

Every test sets the contraction mode itself and restores it (and set_halo) in a finally; nothing here depends on FF_GEMM.

Elsewhere: the kernels that round an intermediate no test can observe -- token_mlp, token_projmlp, token_linear_gated on unmoved
inputs, naf_ffn, naf_front, naf_tail, sgfn_tail -- are held to the same fp32 bound by tests/test_lowprec_fused_gpu.py, against
stage-rounded fp64 references (tests/golden/stage_ref.py) that account for the roundings fp32 noise can flip.  The attention kernels
are held to tests/golden/attn_ref.py by tests/test_lowprec_attn_gpu.py; chan_qkv to tests/golden/chan_ref.py by tests/test_chan_attn_gpu.py.  naf_tail's anchor, ops.linear(kmul=...) in plain bf16, is pinned here.

Two departures from a literal reading of the case list, both forced by ops.conv2d's own rules:
  * 180 -> 180 at 33x20 (one of the five ragged shapes of test_plain_bf16_forms_of_the_fused_kernels) has 660 pixels; conv2d gives the
    LDS-resident kernel images of 1024 pixels and more, so this shape runs -- there as here -- the implicit GEMM.  It is kept, with that
    route asserted, and 180 -> 180 at 33x32 is added so that the form is also exercised ragged in the halo kernel.
  * bf16 input / output rows exist without a residual only (conv2d raises otherwise); those cases use act, mul and alpha."""
import contextlib
import json
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from lowprec_ref import FP32_CHAIN_TOL as TOL  # noqa: E402  (2e-5 of max(1, max|ref|): the bound of an fp32 accumulation chain)

MODES = ["bf16", "bf16x2"]
WORST = {}                    # family -> mode -> worst err / max(1, max|ref|) seen in this run (printed when the module finishes)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isr2_amd import lib
    lib.load()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    yield torch.device("cuda:0")
    print("\nLOWPREC_WORST " + json.dumps(WORST, sort_keys=True))


@contextlib.contextmanager
def _mode(mode, halo=True):
    """Contraction mode (and the halo switch) for one test body, restored in a finally."""
    from isr2_amd import ops
    prev = ops.gemm_mode()
    ops.set_gemm_mode(mode)
    ops.set_halo(halo)
    try:
        yield ops
    finally:
        ops.set_halo(True)
        ops.set_gemm_mode(prev)


def rnd(*shape, dev, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def _note(family, mode, err):
    fam = WORST.setdefault(family, {})
    fam[mode] = max(fam.get(mode, 0.0), err)


def _check(out, ref, family, mode, name, tol=TOL):
    import lowprec_ref as R
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(ref.shape), (name, out.dtype, tuple(out.shape), tuple(ref.shape))
    err = R.rel_err(out, ref)
    _note(family, mode, err)
    print(f"{family} [{mode}] {name}: err = {err:.3e} of max(1, max|ref| = {ref.abs().max().item():.3e})")
    assert err <= tol, f"{family} [{mode}] {name}: {err:.3e} > {tol:.1e}"


def _assert_igemm_route(ops, w, mode, dynamic=False):
    """The call went through ff_conv2d_bf16s with this mode's term count: the weight's prepared image is the hi plane alone."""
    for kind in ("halo", "halo1", "small"):
        assert ops.PREPARED.peek(w, kind) is None, f"{kind} kernel was selected"
    ent = ops.PREPARED.peek(w, "split")
    if dynamic:
        assert ent is None, "a dynamic weight must not be cached"
        return
    assert ent is not None, "the implicit GEMM was not selected (no split image was prepared)"
    assert ent[4] == ops.GEMM_MODES[mode] and ent[1] is None, (ent[4], ent[1] is None)


def _conv_case(dev, mode, family, name, B, H, W, Cin, Cout, k, s, p, act=None, with_res=False, with_mul=False, alpha=1.0, shuffle=0,
               hint=0, dynamic=False, halo=False, seed=0):
    """One ops.conv2d call through the implicit GEMM against the operand-rounded fp64 convolution."""
    import lowprec_ref as R
    from isr2_amd.prep import pack_conv
    x = rnd(B, H, W, Cin, dev=dev, seed=seed + 1)
    w = rnd(Cout, Cin, k, k, dev=dev, seed=seed + 2, scale=1.0 / math.sqrt(Cin * k * k))
    b = rnd(Cout, dev=dev, seed=seed + 3, scale=0.1)
    mul = rnd(Cout, dev=dev, seed=seed + 4) if with_mul else None
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    oshape = (B, 2 * Ho, 2 * Wo, Cout // 4) if shuffle == 2 else (B, Ho, Wo, Cout)
    res = rnd(*oshape, dev=dev, seed=seed + 5) if with_res else None
    wp = pack_conv(w)
    with _mode(mode, halo=halo) as ops:
        out = ops.conv2d(x, wp, b, ksize=(k, k), stride=(s, s), pad=(p, p), act=act, res=res, mul=mul, alpha=alpha, shuffle=shuffle,
                         tile_hint=hint, dynamic_w=dynamic)
        _assert_igemm_route(ops, wp, mode, dynamic)
    ref = R.epilogue_f64(R.conv_taps_f64(R.operand_a(x, mode), R.operand_w(w), s, p), b, act, mul, alpha, res, shuffle=shuffle)
    _check(out, ref, family, mode, name)


# ---------------------------------------------------------------------------------------------------------------------
# Implicit GEMM (ff_conv2d_bf16s, NTERMS = 1 and 2)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,H,W,Cin,Cout,k,s,p,act", [
    (1, 16, 16, 180, 180, 3, 1, 1, None),      # RHAG conv
    (1, 19, 23, 180, 60, 3, 1, 1, "gelu"),     # CAB conv1, ragged M
    (1, 16, 16, 60, 180, 3, 1, 1, None),
    (2, 12, 20, 3, 64, 3, 1, 1, "relu"),       # scalar path (Cin=3)
    (1, 16, 16, 73, 64, 3, 1, 1, "gelu"),      # scalar path (Cin=73)
    (1, 32, 32, 64, 128, 2, 2, 0, None),       # NAFNet down
    (1, 16, 16, 64, 3, 3, 1, 1, "sigmoid"),    # tiny Cout
    (1, 8, 8, 1024, 2048, 1, 1, 0, None),      # 128x128 tile config
    (1, 24, 24, 32, 1, 3, 1, 1, "sigmoid"),
])
def test_conv2d_shapes(dev, mode, B, H, W, Cin, Cout, k, s, p, act):
    """The nine shapes of test_conv2d_matches_torch, activations included."""
    _conv_case(dev, mode, "igemm/conv2d", f"{Cin}->{Cout} k{k}s{s} {H}x{W} {act}", B, H, W, Cin, Cout, k, s, p, act=act, seed=10)


TILE_SHAPES = [(4096, 1024, 2048, 1), (1111, 192, 200, 1), (900, 180, 96, 1), (30 * 30, 64, 130, 3), (24 * 24, 128, 64, 2)]


def _tile_case(dev, mode, hint, M, K, N, k, family):
    hw = int(round(math.sqrt(M))) if k > 1 else None
    B, H, W = (1, hw, hw) if k > 1 else (1, 1, M)
    st, pd = (2, 0) if k == 2 else (1, k // 2)
    _conv_case(dev, mode, family, f"hint {hint} M{M} K{K} N{N} k{k}", B, H, W, K, N, k, st, pd, with_res=True, with_mul=True, hint=hint, seed=120)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hint", [1, 2, 3, 4, 5, 6, 7, 8, 9])
@pytest.mark.parametrize("M,K,N,k", TILE_SHAPES)
def test_gemm_tile_forms(dev, mode, hint, M, K, N, k):
    """Every tile form (4- and 8-wave tiles, 32- and 64-deep chunks) on ragged and exact shapes, 1x1 / 3x3 / 2x2-stride-2, with residual and
    per-channel scale.  All five shapes pad to 64 per tap, so hints 8 and 9 run 64-deep here; their fallback is the next test."""
    _tile_case(dev, mode, hint, M, K, N, k, "igemm/tile_forms")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hint", [8, 9])
@pytest.mark.parametrize("M,K,N,k", [(700, 160, 72, 1),      # Cp = 160: not a multiple of 64 -> 32-deep form
                                     (500, 96, 200, 1),      # Kp = 96
                                     (26 * 26, 96, 130, 3),  # per-tap Cp = 96, 3x3
                                     (600, 73, 64, 1)])      # Cin % 4 != 0: scalar staging, flat K, Kp = 96
def test_gemm_tile_hint_64_deep_fallback(dev, mode, hint, M, K, N, k):
    """Hints 8 / 9 on shapes whose K does not pad to 64: the launcher falls back to the 32-deep forms 5 / 7."""
    _tile_case(dev, mode, hint, M, K, N, k, "igemm/tile_forms")


def _linear_case(dev, mode, family, M, K, N, act=None, with_res=False, with_mul=False, kmul=False, dynamic=False, seed=200):
    import lowprec_ref as R
    x = rnd(M, K, dev=dev, seed=seed)
    w = rnd(N, K, dev=dev, seed=seed + 1, scale=1.0 / math.sqrt(K))
    b = rnd(N, dev=dev, seed=seed + 2, scale=0.1)
    res = rnd(M, N, dev=dev, seed=seed + 3) if with_res else None
    mul = rnd(N, dev=dev, seed=seed + 4) if with_mul else None
    km = (rnd(K, dev=dev, seed=seed + 5) * 0.5 + 1.0).contiguous() if kmul else None
    with _mode(mode) as ops:
        out = ops.linear(x, w, b, act=act, res=res, mul=mul, kmul=km, dynamic_w=dynamic)
        _assert_igemm_route(ops, w, mode, dynamic)
    ref = R.epilogue_f64(R.operand_a(x, mode, km).matmul(R.operand_w(w).t()), b, act, mul, 1.0, res)
    _check(out, ref, family, mode, f"M{M} K{K} N{N} act={act} res={with_res} mul={with_mul} kmul={kmul}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,K,N", [(65536, 360, 180), (65536, 320, 360), (65536, 384, 540), (65536, 180, 540), (16384 + 37, 720, 180)])
def test_linear_at_bench_size(dev, mode, M, K, N):
    """The five shapes of test_linear_at_bench_size (the 256x192 tile and its thresholds), GELU + residual."""
    _linear_case(dev, mode, "igemm/bench_size", M, K, N, act="gelu", with_res=True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,K,N", [(65536, 256, 512), (16384, 512, 1024), (4096, 1024, 2048), (4096, 1024, 1024), (16384 + 19, 512, 1024)])
def test_linear_at_nafnet_deep_levels(dev, mode, M, K, N):
    """NAFNet's deep levels of the bench tile (c = 256 / 512 / 1024): conv1-sized and conv5-sized GEMMs, the latter's per-channel scale +
    residual epilogue, and one ragged M just above 16384."""
    _linear_case(dev, mode, "igemm/bench_size", M, K, N, with_res=True, with_mul=True, seed=260)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,K,N", [(4096, 1024, 2048), (1000, 256, 512), (333, 64, 128), (65536, 256, 512)])
def test_linear_kmul_and_gate_pairs(dev, mode, M, K, N):
    """NAFBlock's two GEMM fusions: conv3(x * sca) as a scale on the A operand -- applied BEFORE the rounding, in fp32 -- with beta and the
    residual in the epilogue, and conv4 + SimpleGate on interleaved rows, also into a channel slice of a wider buffer."""
    import lowprec_ref as R
    _linear_case(dev, mode, "igemm/kmul", M, K, N, with_res=True, with_mul=True, kmul=True, seed=130)
    x = rnd(M, K, dev=dev, seed=130)
    w = rnd(N, K, dev=dev, seed=131, scale=1.0 / math.sqrt(K))
    b = rnd(N, dev=dev, seed=132, scale=0.1)
    c = N // 2
    wi = torch.stack((w[:c], w[c:]), dim=1).reshape(N, K).contiguous()
    bi = torch.stack((b[:c], b[c:]), dim=1).reshape(-1).contiguous()
    wide = torch.full((M, c + 12), 7.0, device=dev)
    with _mode(mode) as ops:
        got = ops.linear(x, wi, bi, gate_pairs=True)
        _assert_igemm_route(ops, wi, mode)
        ops.linear(x, wi, bi, gate_pairs=True, out=wide[:, 4:4 + c])
    y = R.operand_a(x, mode).matmul(R.operand_w(w).t()) + b.double()
    ref = y[:, :c] * y[:, c:]                                          # the chunk(2) halves of the un-interleaved weight
    inter = R.epilogue_f64(R.operand_a(x, mode).matmul(R.operand_w(wi).t()), bi, gate_pairs=True)     # the same from the interleaved rows
    assert (ref - inter).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())
    _check(got, ref, "igemm/gate_pairs", mode, f"M{M} K{K} N{N}")
    assert torch.equal(wide[:, 4:4 + c], got), "the slice write differs from the contiguous one"
    assert (wide[:, :4] == 7.0).all() and (wide[:, 4 + c:] == 7.0).all(), "neighbouring channels were touched"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("Cin,hw", [(64, 1024), (512, 128)])
def test_nafnet_downs(dev, mode, Cin, hw):
    """NAFNet's downs: 2x2 stride-2 convolutions C -> 2C at the bench tile's first and fourth level."""
    _conv_case(dev, mode, "igemm/downs", f"{Cin}->{2 * Cin} {hw}x{hw}", 1, hw, hw, Cin, 2 * Cin, 2, 2, 0, seed=300)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("Cin,hw", [(1024, 64), (128, 512)])
def test_nafnet_ups(dev, mode, Cin, hw):
    """NAFNet's ups: 1x1 C -> 2C, PixelShuffle(2) in the epilogue, plus the skip connection as the residual of the shuffled output."""
    _conv_case(dev, mode, "igemm/ups", f"{Cin}->{2 * Cin} {hw}x{hw} shuffle", 1, hw, hw, Cin, 2 * Cin, 1, 1, 0, with_res=True, shuffle=2, seed=310)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("Cin,H,W,act", [(3, 1024, 1024, None), (73, 37, 45, "gelu")])
def test_intro_flat_k(dev, mode, Cin, H, W, act):
    """NAFNet's intro (3 -> 64, 3x3, at the bench tile's 1024x1024) and Cin = 73 at a ragged size: flat K order, scalar staging, K tail."""
    _conv_case(dev, mode, "igemm/intro", f"{Cin}->64 {H}x{W}", 1, H, W, Cin, 64, 3, 1, 1, act=act, seed=320)


@pytest.mark.parametrize("mode", MODES)
def test_conv2d_epilogue_residual_mul_alpha_and_slices(dev, mode):
    """Input a channel slice [10:74] of a wider buffer (unaligned rows: scalar staging), output into the slice [16:80] of another."""
    import lowprec_ref as R
    from isr2_amd.prep import pack_conv
    B, H, W, Cin, Cout = 1, 20, 20, 64, 64
    wide = rnd(B, H, W, 100, dev=dev, seed=4)
    x = wide[..., 10:74]
    w = rnd(Cout, Cin, 1, 1, dev=dev, seed=5, scale=0.1)
    b = rnd(Cout, dev=dev, seed=6, scale=0.1)
    mul = rnd(Cout, dev=dev, seed=7)
    res = rnd(B, H, W, Cout, dev=dev, seed=8)
    obuf = torch.full((B, H, W, 96), 7.0, device=dev)
    wp = pack_conv(w)
    with _mode(mode) as ops:
        out = ops.conv2d(x, wp, b, act="lrelu", res=res, mul=mul, alpha=0.3, out=obuf[..., 16:80])
        _assert_igemm_route(ops, wp, mode)
    ref = R.epilogue_f64(R.conv_taps_f64(R.operand_a(x.contiguous(), mode), R.operand_w(w)), b, "lrelu", mul, 0.3, res)
    _check(out.contiguous(), ref, "igemm/slices", mode, "slice in / slice out")
    assert (obuf[..., :16] == 7.0).all() and (obuf[..., 80:] == 7.0).all(), "neighbouring channels were touched"


@pytest.mark.parametrize("mode", MODES)
def test_dynamic_weight(dev, mode):
    """dynamic_w=True: the weight is split on every call and never cached (a 1x1 GEMM, and a 3x3 the halo kernel must decline)."""
    _linear_case(dev, mode, "igemm/dynamic_w", 1000, 180, 540, act="gelu", dynamic=True, seed=12)
    _conv_case(dev, mode, "igemm/dynamic_w", "64->64 3x3 40x40 dynamic", 1, 40, 40, 64, 64, 3, 1, 1, dynamic=True, halo=True, seed=330)


@pytest.mark.parametrize("mode", MODES)
def test_conv3x3_at_bench_size_halo_off(dev, mode):
    """180 -> 180 3x3 on the bench tile's 256x256 token grid through the implicit GEMM's large-M tile."""
    _conv_case(dev, mode, "igemm/conv3x3_256", "180->180 256x256", 1, 256, 256, 180, 180, 3, 1, 1, with_res=True, seed=210)


# ---------------------------------------------------------------------------------------------------------------------
# LDS-resident 3x3 convolution (ff_conv3x3_halo, NTERMS = 1)
def _halo_case(dev, family, B, H, W, Cin, Cout, act, expect_halo=True, seed=60):
    """act, residual, per-channel scale, alpha and a strided input view; the pool from the same launch (scalar epilogue, residual included)
    and from a launch without residual (vector epilogue)."""
    import lowprec_ref as R
    from isr2_amd.prep import pack_conv
    mode = "bf16"
    wide = rnd(B, H, W, Cin + 8, dev=dev, seed=seed)
    x = wide[..., 4:4 + Cin]
    w = rnd(Cout, Cin, 3, 3, dev=dev, seed=seed + 1, scale=1.0 / math.sqrt(9 * Cin))
    b = rnd(Cout, dev=dev, seed=seed + 2, scale=0.1)
    mul = rnd(Cout, dev=dev, seed=seed + 3)
    res = rnd(B, H, W, Cout, dev=dev, seed=seed + 4)
    wp = pack_conv(w)
    name = f"{Cin}->{Cout} {B}x{H}x{W} {act}"
    with _mode(mode) as ops:
        out = ops.conv2d(x, wp, b, ksize=(3, 3), pad=(1, 1), act=act, res=res, mul=mul, alpha=0.7)
        if expect_halo:
            assert ops.PREPARED.peek(wp, "halo1") is not None, "the plain-bf16 halo kernel was not selected"
            assert ops.PREPARED.peek(wp, "halo") is None and ops.PREPARED.peek(wp, "split") is None
        else:
            _assert_igemm_route(ops, wp, mode)
        pooled = nores = None
        if B == 1:
            out3, pooled = ops.conv2d(x, wp, b, ksize=(3, 3), pad=(1, 1), act=act, res=res, mul=mul, alpha=0.7, want_pool=True)
            nores = ops.conv2d(x, wp, b, ksize=(3, 3), pad=(1, 1), act=act, mul=mul, alpha=0.7, want_pool=True)
    y = R.conv_taps_f64(R.operand_a(x.contiguous(), mode), R.operand_w(w), 1, 1)
    ref = R.epilogue_f64(y, b, act, mul, 0.7, res)
    _check(out, ref, family, mode, name)
    if B == 1:
        assert torch.equal(out3, out), "want_pool changed the stored output"
        _check(pooled, ref.mean(dim=(1, 2)), family + "/pool", mode, name + " pool (with residual)")
        ref0 = R.epilogue_f64(y, b, act, mul, 0.7, None)
        _check(nores[0], ref0, family, mode, name + " (no residual)")
        _check(nores[1], ref0.mean(dim=(1, 2)), family + "/pool", mode, name + " pool (no residual)")


@pytest.mark.parametrize("B,H,W,Cin,Cout,act", [
    (1, 48, 48, 180, 60, "gelu"),      # CAB conv1: 3 channel chunks, bn 64 (16x16-pixel tiles)
    (2, 37, 45, 128, 180, "relu"),     # ragged tiles, batch 2, bn 192 (8x16 tiles)
    (1, 40, 33, 180, 180, "lrelu"),    # RHAG conv
    (1, 64, 64, 64, 3, "sigmoid"),     # bn 32
    (1, 35, 64, 128, 128, "gelu"),     # bn 128
    (1, 32, 32, 128, 256, "relu"),     # two 128-wide n-blocks
    (1, 32, 40, 36, 40, "lrelu"),      # Cin < 64 (zero-padded chunk), ragged n-block
    (1, 32, 40, 132, 200, "gelu"),     # ragged last chunk, two ragged n-blocks
    # the ragged shapes of test_plain_bf16_forms_of_the_fused_kernels: every launch form
    (1, 37, 45, 180, 60, "gelu"),
    (1, 40, 33, 60, 180, "sigmoid"),
    (1, 33, 32, 180, 180, "relu"),     # (added: 33x20 below is too small for the halo kernel)
    (1, 64, 70, 76, 64, "lrelu"),
    (1, 50, 40, 64, 32, "gelu"),
])
def test_conv3x3_halo(dev, B, H, W, Cin, Cout, act):
    _halo_case(dev, "halo/conv3x3", B, H, W, Cin, Cout, act)


def test_conv3x3_below_the_halo_threshold_takes_the_implicit_gemm(dev):
    """180 -> 180 at 33x20 = 660 pixels: ops.conv2d keeps the LDS-resident kernel for images of 1024 pixels and more."""
    _halo_case(dev, "igemm/conv2d", 1, 33, 20, 180, 180, "gelu", expect_halo=False)


@pytest.mark.parametrize("Cin,Cout,hw", [(180, 180, 256), (180, 60, 256), (64, 64, 512), (76, 64, 256)])
def test_conv3x3_halo_at_bench_size(dev, Cin, Cout, hw):
    """The bench tile's grids: 256x256 tokens (HAT / DAT) and 512x512 (fusion stack); pool partials over 256+ workgroups."""
    _halo_case(dev, "halo/bench_size", 1, hw, hw, Cin, Cout, "gelu", seed=210)


@pytest.mark.parametrize("H,W,Cin,Cout,act", [(48, 48, 180, 60, "gelu"), (40, 33, 60, 180, None), (37, 45, 180, 180, "lrelu"), (64, 64, 64, 32, "sigmoid")])
def test_conv3x3_halo_bf16_rows(dev, H, W, Cin, Cout, act):
    """bf16 input rows are upcast exactly (they ARE the A operand); bf16 output rows are within half a bf16 ulp + the fp32 bound."""
    import lowprec_ref as R
    from isr2_amd.prep import pack_conv
    mode = "bf16"
    x = rnd(1, H, W, Cin, dev=dev, seed=400)
    w = rnd(Cout, Cin, 3, 3, dev=dev, seed=401, scale=1.0 / math.sqrt(9 * Cin))
    b = rnd(Cout, dev=dev, seed=402, scale=0.1)
    mul = rnd(Cout, dev=dev, seed=403)
    wp = pack_conv(w)
    with _mode(mode) as ops:
        x16 = ops.empty_rows_bf16((1, H, W, Cin), dev)
        x16.copy_(x)
        o_f = ops.conv2d(x16, wp, b, ksize=(3, 3), pad=(1, 1), act=act, mul=mul, alpha=0.7)
        o_h = ops.conv2d(x16, wp, b, ksize=(3, 3), pad=(1, 1), act=act, mul=mul, alpha=0.7, out_bf16=True)
        o_fh = ops.conv2d(x, wp, b, ksize=(3, 3), pad=(1, 1), act=act, mul=mul, alpha=0.7, out_bf16=True)
        assert ops.PREPARED.peek(wp, "halo1") is not None and ops.PREPARED.peek(wp, "split") is None
    assert x16.dtype == torch.bfloat16 and o_h.dtype == torch.bfloat16 and o_fh.dtype == torch.bfloat16
    name = f"{Cin}->{Cout} {H}x{W} {act}"
    ref = R.epilogue_f64(R.conv_taps_f64(x16.double().contiguous(), R.operand_w(w), 1, 1), b, act, mul, 0.7, None)
    _check(o_f, ref, "halo/bf16_rows", mode, name + " bf16 in, fp32 out")
    for o, r, tag in ((o_h, ref, "bf16 in, bf16 out"),
                      (o_fh, R.epilogue_f64(R.conv_taps_f64(R.operand_a(x, mode), R.operand_w(w), 1, 1), b, act, mul, 0.7, None), "fp32 in, bf16 out")):
        exc = R.bf16_row_excess(o, r, TOL)
        print(f"halo/bf16_rows [{mode}] {name} {tag}: max(|d| - (2^-8 |ref| + {TOL:.0e} max(1, max|ref|))) = {exc:.3e}")
        assert tuple(o.shape) == tuple(r.shape) and exc <= 0.0, (tag, exc)
    # the stored bf16 value is the RNE rounding of the fp32 value the other launch stored
    assert torch.equal(o_h.float(), R.bf16_rne(o_f)), "bf16 output rows are not the rounded fp32 rows"


@pytest.mark.parametrize("H,W", [(256, 256), (48, 64), (37, 45), (33, 32), (40, 100)])
def test_cab_pair_launch_by_launch(dev, H, W):
    """HAT's CAB: conv3x3 180 -> 60 with GELU, then conv3x3 60 -> 180 with the pool from its epilogue.  The second launch's reference is
    built from the first launch's ACTUAL output, so each launch is held to the fp32 bound on its own; also with conv1's rows in bf16."""
    import lowprec_ref as R
    from isr2_amd.prep import pack_conv
    C, Cm, mode = 180, 60, "bf16"
    x = torch.empty(1, H, W, 192, device=dev)[..., :C]
    x.copy_(rnd(1, H, W, C, dev=dev, seed=1100, scale=1.2) + 0.1)
    w1, b1 = rnd(Cm, C, 3, 3, dev=dev, seed=1101, scale=1.0 / math.sqrt(9 * C)), rnd(Cm, dev=dev, seed=1102, scale=0.2)
    w2, b2 = rnd(C, Cm, 3, 3, dev=dev, seed=1103, scale=1.0 / math.sqrt(9 * Cm)), rnd(C, dev=dev, seed=1104, scale=0.2)
    w1p, w2p = pack_conv(w1), pack_conv(w2)
    with _mode(mode) as ops:
        c1 = ops.conv2d(x, w1p, b1, ksize=(3, 3), pad=(1, 1), act="gelu")
        got, pooled = ops.conv2d(c1, w2p, b2, ksize=(3, 3), pad=(1, 1), want_pool=True)
        c1h = ops.conv2d(x, w1p, b1, ksize=(3, 3), pad=(1, 1), act="gelu", out_bf16=True)
        got_h, pooled_h = ops.conv2d(c1h, w2p, b2, ksize=(3, 3), pad=(1, 1), want_pool=True)
        assert ops.PREPARED.peek(w1p, "halo1") is not None and ops.PREPARED.peek(w2p, "halo1") is not None
        assert ops.PREPARED.peek(w1p, "split") is None and ops.PREPARED.peek(w2p, "split") is None
    ref1 = R.epilogue_f64(R.conv_taps_f64(R.operand_a(x.contiguous(), mode), R.operand_w(w1), 1, 1), b1, "gelu")
    _check(c1.contiguous(), ref1, "halo/cab", mode, f"{H}x{W} conv1 + GELU")
    ref2 = R.epilogue_f64(R.conv_taps_f64(R.operand_a(c1.contiguous(), mode), R.operand_w(w2), 1, 1), b2)
    _check(got.contiguous(), ref2, "halo/cab", mode, f"{H}x{W} conv2 from conv1's actual output")
    _check(pooled, ref2.mean(dim=(1, 2)), "halo/cab", mode, f"{H}x{W} pooled")
    assert torch.equal(c1h.float(), R.bf16_rne(c1.contiguous())), "conv1's bf16 rows are not its rounded fp32 rows"
    assert torch.equal(got_h, got) and torch.equal(pooled_h, pooled), "bf16 conv1 rows changed conv2 (its A operand is the same)"


# ---------------------------------------------------------------------------------------------------------------------
# token_linear / token_linear_gated (NTERMS = 1)
@pytest.mark.parametrize("nres", [1, 2])
@pytest.mark.parametrize("N", [11, 180, 182, 540])
@pytest.mark.parametrize("M", [77, 1000, 65536])
def test_token_linear_projection(dev, M, N, nres):
    """Without LayerNorm: proj + one or two residuals; the A operand is bf16_rne(x).  N = 11 / 182 take the scalar store path."""
    import lowprec_ref as R
    from isr2_amd.prep import pack_token_linear
    C, mode = 180, "bf16"
    x = torch.empty(M, 192, device=dev)[:, :C]
    x.copy_(rnd(M, C, dev=dev, seed=100, scale=1.5) + 0.3)
    w, bias = rnd(N, C, dev=dev, seed=103, scale=1.0 / math.sqrt(C)), rnd(N, dev=dev, seed=104, scale=0.1)
    res, res2, rs2 = rnd(M, N, dev=dev, seed=105), rnd(M, N, dev=dev, seed=106), rnd(N, dev=dev, seed=107)
    with _mode(mode) as ops:
        out = ops.token_linear(x, pack_token_linear(w, bias), res=res, res2=res2 if nres == 2 else None, res2_scale=rs2 if nres == 2 else None)
    ref = R.operand_a(x.contiguous(), mode).matmul(R.operand_w(w).t()) + bias.double() + res.double()
    if nres == 2:
        ref = ref + res2.double() * rs2.double()
    _check(out.contiguous(), ref, "token_linear/proj", mode, f"M{M} N{N} nres{nres}")


@pytest.mark.parametrize("M,K,N,eps,act,stats", [(65536, 180, 540, 1e-5, None, None), (777, 180, 720, 1e-5, "gelu", None),
                                                 (3000, 180, 720, 1e-5, "gelu", (360, 720)), (65536, 180, 720, 1e-5, "gelu", (360, 720)),
                                                 (77, 180, 180, 1e-5, None, None), (5000, 64, 128, 1e-6, None, None),
                                                 (5000, 128, 256, 1e-6, "gelu", None)])
def test_token_linear_layernorm(dev, M, K, N, eps, act, stats):
    """With the LayerNorm prologue.  The kernel stores the fp32 value it then rounds as the xn side output, so the reference operand is
    bf16_rne(xn returned) -- no rounding flips from a differently rounded LayerNorm -- and xn itself is checked against an fp64 LayerNorm.
    GELU is the tanh form in this mode (ff_gelu_sig2).  stats_range: the (mean, rstd) side output of the activated channels."""
    import lowprec_ref as R
    from isr2_amd.prep import pack_token_linear
    mode = "bf16"
    x = rnd(M, K, dev=dev, seed=100, scale=1.5) + 0.3
    g, b = rnd(K, dev=dev, seed=101) * 0.1 + 1, rnd(K, dev=dev, seed=102) * 0.1
    w, bias = rnd(N, K, dev=dev, seed=103, scale=1.0 / math.sqrt(K)), rnd(N, dev=dev, seed=104, scale=0.1)
    res = rnd(M, N, dev=dev, seed=105)
    pk = pack_token_linear(w, bias)
    with _mode(mode) as ops:
        out, xn = ops.token_linear(x, pk, gamma=g, beta=b, eps=eps, act=act, res=res, want_xn=True)
        if stats is not None:
            out_s, st = ops.token_linear(x, pk, gamma=g, beta=b, eps=eps, act=act, res=res, stats_range=stats)
    xn = xn.contiguous()
    _check(xn, R.layernorm_f64(x, g, b, eps), "token_linear/xn", mode, f"M{M} K{K} xn side output", tol=1e-5)
    act_ref = R.act_f64(R.bf16_rne(xn).double().matmul(R.operand_w(w).t()) + bias.double(), act, gelu="tanh")
    _check(out.contiguous(), act_ref + res.double(), "token_linear/ln", mode, f"M{M} K{K} N{N} act={act}")
    if stats is not None:
        assert torch.equal(out_s, out), "the statistics side output changed the result"
        seg = act_ref[:, stats[0]:stats[1]]
        _check(st[:, 0].contiguous(), seg.mean(-1), "token_linear/stats", mode, f"M{M} token mean")
        # the kernel forms var = E[v^2] - mean^2 in fp32: the fp32-chain bound on E[v^2], amplified by the cancellation E[v^2] / (var + eps);
        # rstd = (var + eps)^-1/2 moves by half of that relative error
        var = seg.var(-1, unbiased=False)
        rstd = 1.0 / torch.sqrt(var + 1e-5)
        rel = (st[:, 1].double() - rstd).abs() / rstd
        bound = 0.5 * TOL * seg.pow(2).mean(-1).clamp_min(1.0) / (var + 1e-5)
        print(f"token_linear/stats [{mode}] M{M} rstd: max relative error {rel.max().item():.3e}, smallest bound {bound.min().item():.3e}")
        assert (rel <= bound).all(), (rel - bound).max().item()


def _rounding_candidates(a, o, sm, dsm):
    """Elements of the mix a + o * sm (fp64) that lie within the kernel's own error of a bf16 rounding midpoint: |o| dsm for the gate's
    error, 2^-23 (|a| + |o sm|) for the one or two fp32 roundings of the mix (fma or not)."""
    c = o.double() * sm
    f = a + c
    delta = o.double().abs() * dsm + 2.0 ** -23 * (a.abs() + c.abs())
    ulp = torch.exp2(torch.floor(torch.log2(f.abs().clamp_min(1e-30))) - 7.0)
    t = f.abs() / ulp
    return ((t - torch.floor(t)) - 0.5).abs() * ulp <= 4.0 * delta


@pytest.mark.parametrize("M", [77, 1000, 65536])
def test_token_linear_gated(dev, M):
    """DAT's adaptive interaction + projection: out = res + W (x * cm + x2 * sm) + b, sm = sigmoid(gw2 . gelu(GW1 x + gb1) + gb2).

    The reference builds sm in fp64 from the operands the gate GEMM sees (bf16_rne(x), bf16_rne(GW1)), mixes x * cm + x2 * sm in fp32 and
    rounds.  The kernel's sm is not observable and differs from the fp64 value by up to
        dsm = 1/4 * sum|gw2| * (1.13 * 2e-6 + 1.5e-7) + 4 * 2^-24
    (sigmoid slope <= 1/4; GELU slope <= 1.13; 2e-6 = the fp32-chain error tests/test_lowprec_ref.py holds the accumulation to;
    1.5e-7 = ff_gelu_fast; expf + the rounding of sm itself), so a mix element near a bf16 rounding midpoint could round either way.
    sm depends on x alone, so the test removes the ambiguity from its INPUT instead of allowing for it: wherever the mix would come within
    four times that error of a midpoint, x2 is moved so that the mix sits on the centre of its bf16 cell (set to zero where even the centre
    of so small a cell is too close), and the test asserts that no such element is left.  Every output is then held to the plain 2e-5.
    By construction no element here sits near a tie, so a rounding mode that differs from nearest-even only at ties is not this test's to
    see: test_token_linear_projection has the same staging conversion on unmoved inputs."""
    import lowprec_ref as R
    from isr2_amd.prep import pack_token_linear_gated
    C, Hd, mode = 180, 11, "bf16"
    s = rnd(M, C, dev=dev, seed=800)
    o = rnd(M, C, dev=dev, seed=801)
    cm = torch.sigmoid(rnd(C, dev=dev, seed=803)).contiguous()
    w1, b1 = rnd(Hd, C, dev=dev, seed=804, scale=1.0 / math.sqrt(C)), rnd(Hd, dev=dev, seed=805, scale=0.1)
    w2, b2 = rnd(1, Hd, dev=dev, seed=806, scale=0.5), 0.13
    wp, bp = rnd(C, C, dev=dev, seed=807, scale=1.0 / math.sqrt(C)), rnd(C, dev=dev, seed=808, scale=0.1)
    ga = R.operand_a(s, mode).matmul(R.operand_w(w1).t()) + b1.double()
    sm = torch.sigmoid(R.act_f64(ga, "gelu").matmul(w2.double().t()) + b2)                 # [M, 1], fp64; a function of s alone
    dsm = 0.25 * w2.abs().sum().item() * (1.13 * 2e-6 + 1.5e-7) + 4 * 2.0 ** -24
    a = s.double() * cm.double()
    cand = _rounding_candidates(a, o, sm, dsm)
    moved = cand.double().mean().item()
    centre = R.bf16_rne((a + o.double() * sm).float()).double()
    o = torch.where(cand, ((centre - a) / sm).float(), o)
    o = torch.where(_rounding_candidates(a, o, sm, dsm), torch.zeros_like(o), o)           # the mix is then x * cm alone
    last = _rounding_candidates(a, o, sm, dsm)                                              # x * cm itself on a midpoint: one in ~2^-14 of those
    assert int(last.sum().item()) <= 16
    o = torch.where(last, ((0.5 - a) / sm).float(), o)
    left = int(_rounding_candidates(a, o, sm, dsm).sum().item())
    print(f"token_linear/gated [{mode}] M{M}: {moved:.4f} of the x2 elements moved off a rounding midpoint, {left} left")
    assert left == 0 and moved < 0.05
    sp = torch.empty(M, 192, device=dev)[:, :C]
    sp.copy_(s)
    ch = torch.empty(M, 192, device=dev)[:, :C]
    ch.copy_(o)
    res = torch.empty(M, 192, device=dev)[:, :C]
    res.copy_(rnd(M, C, dev=dev, seed=802))
    with _mode(mode) as ops:
        out = ops.token_linear_gated(sp, ch, pack_token_linear_gated(wp, bp, w1, b1, w2), cm, b2, res=res).contiguous()
    mix32 = s * cm + o * sm.float()                                                         # fp32, as the kernel mixes
    ref = res.contiguous().double() + R.bf16_rne(mix32).double().matmul(R.operand_w(wp).t()) + bp.double()
    _check(out, ref, "token_linear/gated", mode, f"M{M}")
