"""CPU checks of tests/golden/lowprec_ref.py, the operand-rounded fp64 reference that tests/test_lowprec_exact_gpu.py holds the
plain-bf16 and bf16x2 kernels to: the reference has to be right, and its own distance from an fp32 accumulation has to leave
most of the 2e-5 bound to the kernel."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))


def _rnd(*shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def test_bf16_rne_equals_torch_bfloat16():
    import lowprec_ref as R
    x = torch.cat([_rnd(200000, seed=1), _rnd(50000, seed=2, scale=1e-20), _rnd(50000, seed=3, scale=1e20), torch.zeros(4), -torch.zeros(4)])
    # exact ties (low half = 0x8000) on even and odd upper halves, both signs, and the values next to them
    base = torch.tensor([0x3F800000, 0x3F810000, 0x40FF0000, 0x00010000, 0x7F000000], dtype=torch.int64)
    ties = torch.cat([base + d for d in (0x7FFF, 0x8000, 0x8001)])
    ties = torch.cat([ties, ties + 0x80000000])
    ties = torch.where(ties >= 2 ** 31, ties - 2 ** 32, ties).to(torch.int32).view(torch.float32)
    x = torch.cat([x, ties])
    got = R.bf16_rne(x)
    assert torch.equal(got, x.bfloat16().float())
    assert torch.equal(got.view(torch.int32) & 0xFFFF, torch.zeros_like(got, dtype=torch.int32))
    t = R.bf16_trunc(x)
    nrm = x.abs() > 1e-30                                  # (below the normal range an ulp is not a fraction of the value)
    assert (t.abs() <= x.abs()).all() and ((x - t).abs() <= x.abs() * 2.0 ** -7)[nrm].all()
    assert not torch.equal(t, got)


def test_hi_lo_split_reproduces_x_to_2_pow_minus_16():
    import lowprec_ref as R
    x = torch.cat([_rnd(300000, seed=4), _rnd(100000, seed=5, scale=37.0), _rnd(100000, seed=6, scale=1e-3)])
    a = R.split_bf16x2(x)
    assert a.dtype == torch.float64
    assert ((a - x.double()).abs() <= x.double().abs() * 2.0 ** -16).all()
    assert torch.equal(a.float().double(), a), "hi + lo must be an fp32 value"
    assert torch.equal(R.operand_a(x, "bf16x2"), a) and torch.equal(R.operand_a(x, "bf16"), x.bfloat16().double())
    km = _rnd(500000, seed=7) * 0.5 + 1.0
    assert torch.equal(R.operand_a(x, "bf16", kmul=km), (x * km).bfloat16().double())


@pytest.mark.parametrize("k,s,p", [(1, 1, 0), (3, 1, 1), (2, 2, 0)])
def test_tap_sum_convolution_equals_conv2d_fp64(k, s, p):
    import lowprec_ref as R
    x = _rnd(2, 7, 13, 10, seed=8).double()
    w = _rnd(5, 7, k, k, seed=9).double()
    ref = F.conv2d(x, w, stride=s, padding=p).permute(0, 2, 3, 1)
    got = R.conv_taps_f64(x.permute(0, 2, 3, 1).contiguous(), w, stride=s, pad=p)
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() <= 1e-13 * max(1.0, ref.abs().max().item())


def test_epilogue_matches_torch_fp64():
    import lowprec_ref as R
    y = _rnd(2, 5, 6, 16, seed=10).double()
    b, mul = _rnd(16, seed=11), _rnd(16, seed=12)
    res = _rnd(2, 5, 6, 16, seed=13)
    for act, f in (("gelu", F.gelu), ("relu", F.relu), ("lrelu", lambda t: F.leaky_relu(t, 0.01)), ("sigmoid", torch.sigmoid), (None, lambda t: t)):
        ref = res.double() + (mul * 0.7).double() * f(y + b.double())
        assert (R.epilogue_f64(y, b, act, mul, 0.7, res) - ref).abs().max().item() <= 1e-14
    t = F.gelu(y, approximate="tanh")
    assert torch.equal(R.epilogue_f64(y, act="gelu", gelu="tanh"), t)
    yb = y + b.double()
    assert torch.equal(R.epilogue_f64(y, b, gate_pairs=True), yb[..., 0::2] * yb[..., 1::2])
    res2 = _rnd(2, 10, 12, 4, seed=14)
    ref = F.pixel_shuffle(yb.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1) + res2.double()
    assert torch.equal(R.epilogue_f64(y, b, shuffle=2, res=res2), ref)
    x = _rnd(9, 180, seed=15) * 1.5 + 0.3
    g, be = _rnd(180, seed=16) * 0.1 + 1, _rnd(180, seed=17) * 0.1
    ln = F.layer_norm(x.double(), (180,), g.double(), be.double(), 1e-5)
    assert (R.layernorm_f64(x, g, be, 1e-5) - ln).abs().max().item() <= 1e-13


@pytest.mark.parametrize("K", [180, 1620, 2048, 4608])
@pytest.mark.parametrize("mode", ["bf16", "bf16x2"])
def test_reference_alone_stays_inside_the_fp32_bound(mode, K):
    """A 16-deep chunked fp32 accumulation of the rounded operands -- what a correct kernel computes -- against the fp64 reference:
    it must use only a small part of the 2e-5 bound (measured 1e-7 .. 6e-7), so the bound's budget belongs to the kernel."""
    import lowprec_ref as R
    x = _rnd(192, K, seed=20 + K)
    w = _rnd(96, K, seed=21 + K, scale=1.0 / math.sqrt(K))
    a, wt = R.operand_a(x, mode), R.operand_w(w)
    ref = a.matmul(wt.t())
    if mode == "bf16":
        acc = R.chunked_fp32_matmul(a.float(), wt.float())
    else:                                                   # two MFMA terms per chunk into the same accumulator: lo * w, then hi * w
        hi = R.bf16_rne(x)
        lo = R.bf16_rne(x - hi)
        acc = torch.zeros(192, 96)
        for k0 in range(0, K, 16):
            acc = acc + lo[:, k0:k0 + 16].matmul(wt[:, k0:k0 + 16].float().t())
            acc = acc + hi[:, k0:k0 + 16].matmul(wt[:, k0:k0 + 16].float().t())
    err = R.rel_err(acc, ref)
    print(f"reference alone, {mode}, K = {K}: {err:.2e} of max(1, max|ref|)")
    assert err <= R.FP32_CHAIN_TOL
    assert err <= 0.1 * R.FP32_CHAIN_TOL, "the reference's own margin has shrunk: the kernel's share of the bound is no longer ~all of it"
    # and the effect the tests must see through: truncated operands sit far outside the bound
    bad = R.bf16_trunc(x).double().matmul(wt.t())
    assert R.rel_err(bad, ref) > 10 * R.FP32_CHAIN_TOL
