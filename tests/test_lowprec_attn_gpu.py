"""The attention kernels of the plain-bf16 ('bf16') contraction mode against STAGE-ROUNDED fp64 references (tests/golden/attn_ref.py), on
the MI355X: ops.window_attn (window_attn_bf16_kernel<1>, with the expanded biasT table and with rel_table), ops.ocab_attn and
ops.ocab_attn_rows16 (ocab_attn_kernel<false | true>), ops.win_attn_fused (win_attn_fused_v2_kernel<WW, ONES>) -- the single-image entry
points; the `_images` and batched forms are pinned bit for bit against these by tests/test_batched_*_gpu.py.

What held these kernels before was 2e-2 absolute against an fp32 softmax (tests/test_ops_gpu.py, still in place), under which a
dropped key, one wrong bias entry or a denominator summed from the wrong quantity pass.  The reference here rounds where the kernel
rounds -- the un-normalised probability P, relative to the kernel's RUNNING maximum, tile by tile -- and accounts from itself alone for
the probabilities fp32 noise can push across a rounding boundary (attn_ref's docstring: the noise of s and m, a counted budget for the
fma and v_exp_f32, 2^-18 for the scores of masked ONES windows).  The assertion is per element:
    |out - ref| <= 2e-5 * max(1, max|ref|) + allow
with 2e-5 the project's fp32-chain bound (lowprec_ref.FP32_CHAIN_TOL); nothing here is chosen from a kernel's output.  Both caps on the
allowance are asserted before the kernel's output is looked at.  tests/test_attn_ref_cpu.py shows on the CPU that an fp32 stand-in
passes and that a dropped key, a wrong bias gather, an omitted mask, zero keys left out of OCAB's softmax, the wrong denominator rule, a
final-maximum rounding, a 0 instead of -inf tail and a shifted head slice all fail this assertion.

The stand-alone kernels run on randn q / k / v, flat and sharpened; the fused kernel on FIXED-POINT inputs that make every stage ahead
of the exponent exact in fp32 (asserted from the reference), so its v_out side output must equal the fp64 value bit for bit, the bf16 xn
side output the rounded operand, the fp32 one within 2e-6.  The fused kernel on generic inputs stays in tests/test_ops_gpu.py
(test_win_attn_fused_hat / _dat_branches); chan_qkv (its reduction spans the whole image) is held per partial block to
tests/golden/chan_ref.py by tests/test_chan_attn_gpu.py.

Shapes (attn_ref.CASES) are the smallest that reach every path: window_attn HAT 16x16 on 16x16 with shift 8 (one window, every mask
region) and on 32x48 without, OCAB's 24x24 keys on 32x32 (576 keys = 4.5 chunks: the ragged tail; every window has zero keys), DAT 8x32 and
32x8 on 40x72 (padded to 64x96, shifted, masked, channel halves with o_off), odd q_off / o_off (the scalar load and store paths);
ocab_attn on 32x32 and 16x48, fp32 rows and rows16, fp32 and bf16 out, pitches above the row width; win_attn_fused HAT 16x16 shift 8,
32x48 with both xn forms and a bf16 out, the DAT branches with zero_pad, head0 = 3 and v_out, and d = 32 / K = 192 for the non-ONES form.

Measured on MI355X (the line this module prints: per kernel the worst err and err - allow as fractions of max(1, max|ref|), the largest
share of wide allowances and of fragile P).  err reaches 3e-3 where a bf16 output or a probability rounded the other way; err - allow,
what the assertion bounds by 2e-5, stays below 1.1e-6.  Every case takes under half a second, reference included:
    LOWPREC_ATTN_WORST {"ocab_attn": {"err": 0.00323, "err_minus_allow": 7.41e-07, "fragile": 0.00629, "wide": 0.00872}, "win_attn_fused":
    {"err": 0.00106, "err_minus_allow": 4.35e-07, "fragile": 0.00722, "wide": 0.0229}, "window_attn": {"err": 0.00123, "err_minus_allow":
    1.03e-06, "fragile": 0.00738, "wide": 0.00916}}"""
import contextlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import attn_ref as A  # noqa: E402

TOL = A.FP32_CHAIN_TOL
SENT = -3.0                   # what the output buffers hold where the kernel must not write
WORST = {}                    # kernel -> {"err", "err_minus_allow", "wide", "fragile"}: the worst of each seen in this run


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isr2_amd import lib
    lib.load()
    yield torch.device("cuda:0")
    print("\nLOWPREC_ATTN_WORST " + json.dumps({k: {n: float(f"{x:.3g}") for n, x in v.items()} for k, v in WORST.items()}, sort_keys=True))


@contextlib.contextmanager
def _bf16_mode():
    """The plain-bf16 contraction mode for one test body, restored in a finally."""
    from isr2_amd import ops
    prev = ops.gemm_mode()
    ops.set_gemm_mode("bf16")
    try:
        yield ops
    finally:
        ops.set_gemm_mode(prev)


def _reference(kernel, case):
    """Inputs and reference of a case, and the caps -- from the reference alone, before any kernel runs."""
    inp, sr, info = A.reference(kernel, case)
    name = f"{kernel} [{A.case_name(case)}]"
    shares = A.assert_caps(sr, name)
    if kernel == "win_attn_fused":
        A.assert_exact(info["facts"], name)
    return inp, sr, info, shares


def _check(kernel, case, out, sr, info, shares, tag=""):
    w = WORST.setdefault(kernel, dict(err=0.0, err_minus_allow=-1.0, wide=0.0, fragile=0.0))
    err, exc = A.compare(out.float().contiguous().cpu().reshape(sr.shape), sr)
    print(f"{kernel} [{A.case_name(case)}]{tag}: err = {err:.3e}, err - allow = {exc:.3e} of max(1, max|ref| = {sr.ref.abs().max().item():.3e}); "
          f"wide allowances {shares['wide']:.4f}, fragile P {info['fragile']:.4f}")
    w["err"], w["err_minus_allow"] = max(w["err"], err), max(w["err_minus_allow"], exc)
    w["wide"], w["fragile"] = max(w["wide"], shares["wide"]), max(w["fragile"], info["fragile"])
    assert exc <= TOL, f"{kernel} [{A.case_name(case)}]{tag}: err - allow = {exc:.3e} > {TOL:.1e}"


def _cases(kernel):
    return pytest.mark.parametrize("case", A.CASES[kernel], ids=[A.case_name(c).replace(" ", "-") for c in A.CASES[kernel]])


def _untouched(buf, lo, hi):
    """Every channel outside [lo, hi) still holds the sentinel."""
    return bool((buf[..., :lo] == SENT).all()) and bool((buf[..., hi:] == SENT).all())


@_cases("window_attn")
@pytest.mark.parametrize("table", ["biasT", "rel"])
def test_window_attn(dev, case, table):
    """The expanded [heads, keys, 256] table and the compact table gathered in the kernel (rotated for OCAB's overlapping keys)."""
    from isr2_amd.prep import pack_rel_overlap
    inp, sr, info, shares = _reference("window_attn", case)
    heads, d, o_off = inp["heads"], inp["d"], inp["o_off"]
    qkv = inp["qkv"].to(dev)
    out = torch.full((1, inp["H"], inp["W"], A.HEADS * A.D + (2 if case["odd"] else 0)), SENT, device=dev)
    rel = None
    if table == "rel":
        rel = (pack_rel_overlap(inp["rel"].t().contiguous(), 16, 24) if inp["kwin"] != inp["win"] else inp["rel"].contiguous()).to(dev)
    with _bf16_mode() as ops:
        ops.window_attn(qkv, out, A.expand_biasT(inp).to(dev), q_off=inp["q_off"], k_off=inp["k_off"], v_off=inp["v_off"], o_off=o_off, H=inp["H"],
                        W=inp["W"], Hp=inp["Hp"], Wp=inp["Wp"], win=inp["win"], kwin=inp["kwin"], shift=inp["shift"], use_mask=inp["use_mask"],
                        heads=heads, d=d, scale=inp["scale"], rel_table=rel)
    assert _untouched(out, o_off, o_off + heads * d)
    _check("window_attn", case, out[..., o_off:o_off + heads * d], sr, info, shares, f" {table}")


@_cases("ocab_attn")
def test_ocab_attn(dev, case):
    """fp32 rows and the head-padded bf16 rows of token_linear_rows16 (same values), fp32 and bf16 out, pitches above the row width."""
    from isr2_amd.prep import pack_rel_overlap
    inp, sr, info, shares = _reference("ocab_attn", case)
    H, W, C = inp["H"], inp["W"], A.HEADS * A.D
    rel = pack_rel_overlap(inp["rel"].t().contiguous(), 16, 24).to(dev)
    odt = torch.bfloat16 if case["out_bf16"] else torch.float32
    out = torch.full((1, H, W, 192 if case["ld"] else C), SENT, device=dev, dtype=odt)[..., :C]
    with _bf16_mode() as ops:
        if case["rows16"]:
            rows = torch.full((1, H, W, 640 if case["ld"] else 576), 1e30, device=dev, dtype=torch.bfloat16)[..., :576]
            rows.copy_(A.ocab_rows16(inp["qkv"], inp["scale"]))
            ops.ocab_attn_rows16(rows, out, rel, q_off=0, k_off=192, v_off=384, H=H, W=W, heads=A.HEADS, d=A.D, ws=16, ows=24)
        else:
            qkv = torch.full((1, H, W, 3 * C + (12 if case["ld"] else 0)), 1e30, device=dev)[..., :3 * C]
            qkv.copy_(inp["qkv"])
            ops.ocab_attn(qkv, out, rel, q_off=0, k_off=C, v_off=2 * C, H=H, W=W, heads=A.HEADS, d=A.D, ws=16, ows=24, scale=inp["scale"])
    assert out.dtype == odt and (out.stride(2) > C) == case["ld"]
    _check("ocab_attn", case, out, sr, info, shares)


@_cases("win_attn_fused")
def test_win_attn_fused(dev, case):
    """Fixed-point inputs: besides the attention output, the side outputs are exact (v_out, bf16 xn) or within 2e-6 (fp32 xn)."""
    from isr2_amd.prep import pack_win_attn, pack_win_rel
    inp, sr, info, shares = _reference("win_attn_fused", case)
    H, W, d = inp["H"], inp["W"], inp["d"]
    C = A.HEADS * d
    h0, nh = inp["head0"], inp["nheads"]
    x = torch.empty(1, H, W, 192, device=dev)[..., :C]
    x.copy_(inp["x"])
    pk = pack_win_attn(inp["wqkv"].to(dev), inp["bqkv"].to(dev), A.HEADS, d, inp["scale"])
    relp = pack_win_rel(inp["rel"].to(dev), *inp["win"])
    dat = case["kind"] != "hat"
    with _bf16_mode() as ops:
        out = (ops.empty_rows_bf16 if case["out_bf16"] else ops.empty_rows)((1, H, W, C), dev).fill_(SENT)
        vout = torch.full((1, H, W, 3 * C), SENT, device=dev) if dat else None
        res = ops.win_attn_fused(x, out, pk, relp, gamma=inp["gamma"].to(dev), beta=inp["beta"].to(dev), H=H, W=W, Hp=inp["Hp"], Wp=inp["Wp"],
                                 win=inp["win"], shift=inp["shift"], use_mask=inp["use_mask"], head0=h0, nheads=nh, zero_pad=inp["zero_pad"],
                                 want_xn={None: False, "f32": True, "bf16": "bf16"}[case["xn"]], v_out=vout, v_off=2 * C)
    assert _untouched(out, h0 * d, (h0 + nh) * d)
    side = info["side"]
    if case["xn"] == "f32":
        xn = res[1].double().cpu().reshape(H * W, C)
        e = (xn - side["xn"]).abs().max().item() / max(1.0, side["xn"].abs().max().item())
        print(f"win_attn_fused [{A.case_name(case)}] fp32 xn side output: {e:.3e}")
        assert e <= 2e-6
    elif case["xn"] == "bf16":
        assert res[1].dtype == torch.bfloat16 and torch.equal(res[1].double().cpu().reshape(H * W, C), side["xn_bf16"])
    if dat:
        lo = 2 * C + h0 * d
        assert _untouched(vout, lo, lo + nh * d)
        assert torch.equal(vout[..., lo:lo + nh * d].double().cpu().reshape(H * W, nh * d), side["v"]), "v_out is not the exact projection"
    _check("win_attn_fused", case, out[..., h0 * d:(h0 + nh) * d], sr, info, shares)
