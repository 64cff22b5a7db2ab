"""The fused kernels of the plain-bf16 ('bf16') contraction mode against STAGE-ROUNDED fp64 references (tests/golden/stage_ref.py), on
the MI355X: ops.token_mlp, ops.token_projmlp, ops.token_linear_gated, ops.naf_ffn, ops.naf_tail, ops.naf_front, ops.sgfn_tail --
the single-image entry points; the batched `_images` forms and the large-M schedules are pinned bit for bit against these by
tests/test_batched_*_gpu.py and the large-M cases of tests/test_ops_gpu.py / tests/test_naf_tail_gpu.py.

These kernels round an INTERMEDIATE to bf16 (the LayerNorm output, the GELU, a gate product) that no test can observe, which is why
tests/test_lowprec_exact_gpu.py left them on the 2e-2 .. 3e-2 comparison with an fp32 reference.  The reference here rounds where the
kernel rounds -- every cast site is named in stage_ref.py -- and accounts for the intermediates that fp32 noise can push across a
rounding boundary from the reference alone (allowance per output, enumeration of a row's fragile LayerNorm elements; see that module's
docstring).  The assertion is per element and per row:
    |out - ref| <= 2e-5 * max(1, max|ref|) + allow
with 2e-5 the project's fp32-chain bound (lowprec_ref.FP32_CHAIN_TOL), nothing here chosen from a kernel's output: the only measured
constants are the two noise factors of stage_ref.py, four times what an fp32 CPU stand-in gives; the pointwise rounding budgets
next to them are counted from the kernels' source and listed in that module's docstring (tests/test_stage_ref_cpu.py, which
also shows that truncation at any rounding point, the other GELU form, a scale applied after the rounding, a dropped or exchanged
hidden column and a wrong row all fail this assertion on every case below).  The derivable worst case c = K + 8 is not used.  Both
caps on the allowance are asserted before the kernel's output is looked at.

Shapes are the smallest that reach every row path: token kernels (32 rows per wave, 256 per workgroup) M = 77 and 293; naf_ffn /
naf_tail (128-row tiles) M = 77 and 300, naf_tail also on row views with ld > C; naf_front 9x17 and 20x40 (partial 8x16 tiles on both
edges), both outputs; sgfn_tail 8x32 and 19x70, with and without the residual; token_projmlp without c2 and with c2 / c2_scale, with
fp32 and bf16 att / c2 rows (all three non-zero io_bf16 values).

Covered elsewhere: the attention kernels (win_attn_fused in plain bf16, window_attn_bf16s, ocab_attn), whose rounded intermediate is
the softmax probability relative to a running maximum, are held to tests/golden/attn_ref.py by tests/test_lowprec_attn_gpu.py
(win_attn_fused on fixed-point inputs).  chan_qkv (its reduction spans the whole image) is held per partial block to
tests/golden/chan_ref.py by tests/test_chan_attn_gpu.py.  What remains on the checks of tests/test_ops_gpu.py: win_attn_fused on
generic inputs.  The `_images` and batched forms are pinned bit for bit against the single-image forms by
tests/test_batched_*_gpu.py.

Measured on MI355X (the line this module prints: per kernel the worst err and err - allow, both as fractions of max(1, max|ref|), and
the largest allowance shares; figures rounded to three digits here).  err reaches 9e-4 where an intermediate rounded the other way;
err - allow, what the assertion bounds by 2e-5, stays below 2.4e-7:
    LOWPREC_FUSED_WORST {"naf_ffn": {"err": 0.000102, "err_minus_allow": 6.13e-08, "rows_ln": 0.0, "wide": 0.00122}, "naf_front":
    {"err": 1.88e-07, "err_minus_allow": 1.09e-07, "rows_ln": 0.0, "wide": 0.00781}, "naf_tail": {"err": 4.96e-05, "err_minus_allow":
    8.9e-08, "rows_ln": 0.0, "wide": 0.000406}, "sgfn_tail": {"err": 0.000912, "err_minus_allow": 2.38e-07, "rows_ln": 0.0, "wide":
    0.00355}, "token_linear_gated": {"err": 0.000125, "err_minus_allow": 7.67e-08, "rows_ln": 0.0, "wide": 0.0281}, "token_mlp": {"err":
    8.39e-05, "err_minus_allow": 5.54e-10, "rows_ln": 0.0, "wide": 0.00135}, "token_projmlp": {"err": 0.000199, "err_minus_allow":
    -1.12e-08, "rows_ln": 0.013, "wide": 0.0224}}"""
import contextlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import stage_ref as S  # noqa: E402

TOL = S.FP32_CHAIN_TOL
WORST = {}                    # kernel -> {"err", "err_minus_allow", "wide", "rows_ln"}: the worst of each seen in this run


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isr2_amd import lib
    lib.load()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    yield torch.device("cuda:0")
    print("\nLOWPREC_FUSED_WORST " + json.dumps(WORST, sort_keys=True))


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
    """Inputs and reference of a case, and the two caps -- from the reference alone, before any kernel runs."""
    inp, sr = S.reference(kernel, case)
    srs = (sr,) if isinstance(sr, S.StageRef) else tuple(sr)
    shares = [S.assert_caps(r, f"{kernel} [{S.case_name(case)}]" + (" pooled" if i else "")) for i, r in enumerate(srs)]
    return inp, srs, shares


def _to(dev, inp):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}


def _check(kernel, case, outs, srs, shares):
    w = WORST.setdefault(kernel, dict(err=0.0, err_minus_allow=-1.0, wide=0.0, rows_ln=0.0))
    worst = -1.0
    for i, (out, sr, sh) in enumerate(zip(outs, srs, shares)):
        assert out.dtype == torch.float32
        err, exc = S.compare(out.contiguous().cpu(), sr)
        print(f"{kernel} [{S.case_name(case)}]{' pooled' if i else ''}: err = {err:.3e}, err - allow = {exc:.3e} of max(1, max|ref| = "
              f"{sr.ref[0].abs().max().item():.3e}); wide allowances {sh['wide']:.4f}")
        w["err"], w["err_minus_allow"] = max(w["err"], err), max(w["err_minus_allow"], exc)
        w["wide"], w["rows_ln"] = max(w["wide"], sh["wide"]), max(w["rows_ln"], sh["rows_ln"])
        worst = max(worst, exc)
    assert worst <= TOL, f"{kernel} [{S.case_name(case)}]: err - allow = {worst:.3e} > {TOL:.1e}"


def _cases(kernel):
    return pytest.mark.parametrize("case", S.CASES[kernel], ids=[S.case_name(c).replace(" ", "-") for c in S.CASES[kernel]])


@_cases("token_mlp")
def test_token_mlp(dev, case):
    from isr2_amd.prep import pack_token_mlp
    inp, srs, shares = _reference("token_mlp", case)
    d = _to(dev, inp)
    with _bf16_mode() as ops:
        out = ops.token_mlp(d["x"], d["gamma"], d["beta"], pack_token_mlp(d["w1"], d["b1"], d["w2"], d["b2"]))
    _check("token_mlp", case, (out,), srs, shares)


@_cases("token_projmlp")
def test_token_projmlp(dev, case):
    """att / c2 as fp32 rows or as bf16 rows in the padded buffers the attention kernels write (ops.empty_rows_bf16)."""
    from isr2_amd.prep import pack_token_projmlp
    inp, srs, shares = _reference("token_projmlp", case)
    d = _to(dev, inp)
    with _bf16_mode() as ops:
        for name in ("att", "c2"):
            if d.get(name) is not None and d[name].dtype == torch.bfloat16:
                rows = ops.empty_rows_bf16(tuple(d[name].shape), dev)
                rows.copy_(d[name])
                d[name] = rows
        assert (d["att"].dtype == torch.bfloat16) == bool(case["io"] & 1) and (case["c2"] and d["c2"].dtype == torch.bfloat16) == bool(case["io"] & 2)
        out = ops.token_projmlp(d["att"], d["x"], pack_token_projmlp(d["wp"], d["bp"], d["w1"], d["b1"], d["w2"], d["b2"]), d["gamma"], d["beta"],
                                c2=d.get("c2"), c2_scale=d.get("c2_scale"))
    _check("token_projmlp", case, (out,), srs, shares)


@_cases("token_linear_gated")
def test_token_linear_gated(dev, case):
    """DAT's form: hidden 11.  Unlike tests/test_lowprec_exact_gpu.py::test_token_linear_gated the inputs are NOT moved off the
    rounding midpoints: the mix elements the gate's fp32 noise can flip are accounted for by the allowance."""
    from isr2_amd.prep import pack_token_linear_gated
    inp, srs, shares = _reference("token_linear_gated", case)
    d = _to(dev, inp)
    with _bf16_mode() as ops:
        out = ops.token_linear_gated(d["x"], d["x2"], pack_token_linear_gated(d["w"], d["b"], d["gw1"], d["gb1"], d["gw2"]), d["cm"].contiguous(),
                                     d["gb2"], res=d["res"])
    _check("token_linear_gated", case, (out,), srs, shares)


@_cases("naf_ffn")
def test_naf_ffn(dev, case):
    from isr2_amd.prep import pack_naf_ffn
    inp, srs, shares = _reference("naf_ffn", case)
    d = _to(dev, inp)
    with _bf16_mode() as ops:
        out = ops.naf_ffn(d["y"], pack_naf_ffn(d["w4"], d["b4"], d["w5"], d["b5"]), d["ln_g"], d["ln_b"], d["oscale"])
    _check("naf_ffn", case, (out,), srs, shares)


@_cases("naf_tail")
def test_naf_tail(dev, case):
    """views: g and x as channel slices of wider buffers (ld > C, 16-byte aligned rows)."""
    from isr2_amd.prep import pack_naf_tail
    inp, srs, shares = _reference("naf_tail", case)
    d = _to(dev, inp)
    C, M = case["C"], case["M"]
    if case["views"]:
        gbuf, xbuf = torch.full((M, C + 32), 7.0, device=dev), torch.full((M, 2 * C), 7.0, device=dev)
        gbuf[:, 16:16 + C] = d["g"]
        xbuf[:, C:] = d["x"]
        d["g"], d["x"] = gbuf[:, 16:16 + C], xbuf[:, C:]
        assert d["g"].stride(0) > C and d["x"].stride(0) > C
    with _bf16_mode() as ops:
        out = ops.naf_tail(d["g"], d["x"], pack_naf_tail(d["w3"], d["b3"], d["w4"], d["b4"], d["w5"], d["b5"]), d["sca"].contiguous(), d["beta"],
                           d["ln_g"], d["ln_b"], d["gamma"])
    _check("naf_tail", case, (out,), srs, shares)


@_cases("naf_front")
def test_naf_front(dev, case):
    """Both outputs: the gated tensor and its mean over the pixels."""
    from isr2_amd.prep import pack_dw, pack_token_linear
    inp, srs, shares = _reference("naf_front", case)
    d = _to(dev, inp)
    with _bf16_mode() as ops:
        gated, pooled = ops.naf_front(d["x"], pack_token_linear(d["w1"], d["b1"]), d["ln_g"], d["ln_b"], pack_dw(d["wdw"]), d["bdw"])
    _check("naf_front", case, (gated, pooled), srs, shares)


@_cases("sgfn_tail")
def test_sgfn_tail(dev, case):
    from isr2_amd.prep import pack_dw
    inp, srs, shares = _reference("sgfn_tail", case)
    d = _to(dev, inp)
    with _bf16_mode() as ops:
        out = ops.sgfn_tail(d["y"], d["c2"], pack_dw(d["wd"]), d["bd"], d["stats"], d["gamma"], d["beta"], d["w2"], d["b2"], res=d["res"])
    _check("sgfn_tail", case, (out,), srs, shares)
