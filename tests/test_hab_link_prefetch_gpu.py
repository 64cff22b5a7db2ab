"""ops.hab_link and ops.token_projmlp after their loads were moved (csrc/hab_link.hip, csrc/token_mlp.hip): LayerNorm1's gamma / beta, the
hand-over's b2 and the gate row are read from LDS copies, and the residual slices are issued ahead of the slice that is being consumed
(hab_link: two register sets; token_projmlp: one).  No arithmetic statement changed, so

  * ops.hab_link stays bit-equal (torch.equal on x_out, xn, att) to ops.token_projmlp followed by ops.win_attn_fused;
  * ops.token_projmlp -- whose own loop changed, so the pair above is not an independent reference for it -- stays within the pin
    tests' tolerance (tests/golden/stage_ref.py, S.FP32_CHAIN_TOL) of the stage-rounded fp64 reference, in the OCAB form (no c2) and
    the HAB form (c2 and gate), both with the bf16 rows the product hands it.

Shapes are the smallest the link's route accepts (H * W >= 1024, multiples of 16).  16 x 64 is ONE window row, so the shifted row
index wraps onto the same row; 32 x 48 with B = 2 has two different gate rows.  What makes a wrong LDS index or a slice taken from
the wrong register set visible: gamma1, beta1, b2 and the gate differ from channel to channel (and the gate from image to image), the
rows of x and c2 differ from token to token, and the pad columns 180..191 of the att, x and c2 buffers hold NaN -- the kernels never
let them reach a result, so every output must be finite and equal."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import stage_ref as S  # noqa: E402

C, HEADS, D, WS = 180, 6, 30, 16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rnd(*shape, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


class _Bf16Mode:
    def __enter__(self):
        from isr2_amd import ops
        self.prev = ops.gemm_mode()
        ops.set_gemm_mode("bf16")
        return ops

    def __exit__(self, *exc):
        from isr2_amd import ops
        ops.set_gemm_mode(self.prev)


def _nan_padded(ops, values, bf16):
    """`values` in a row buffer of the product's pitch whose pad columns hold NaN."""
    t = ops.empty_rows_bf16(tuple(values.shape), values.device) if bf16 else ops.empty_rows(tuple(values.shape), values.device)
    assert t._base is not None and t._base.shape[-1] >= 192, "the buffer has no pad columns"
    t._base.fill_(float("nan"))
    t.copy_(values)
    assert torch.isnan(t._base[..., C:].float()).all() and torch.isfinite(t.float()).all()
    return t


@pytest.fixture(scope="module")
def weights(dev):
    from isr2_amd.prep import pack_token_projmlp, pack_win_attn, pack_win_rel
    Hd = 2 * C
    pm = pack_token_projmlp(rnd(C, C, dev=dev, seed=2950, scale=1.0 / math.sqrt(C)), rnd(C, dev=dev, seed=2951, scale=0.1),
                            rnd(Hd, C, dev=dev, seed=2952, scale=1.0 / math.sqrt(C)), rnd(Hd, dev=dev, seed=2953, scale=0.1),
                            rnd(C, Hd, dev=dev, seed=2954, scale=1.0 / math.sqrt(Hd)), rnd(C, dev=dev, seed=2955, scale=0.5))      # b2: channel-dependent
    wf = pack_win_attn(rnd(3 * C, C, dev=dev, seed=2956, scale=1.0 / math.sqrt(C)), rnd(3 * C, dev=dev, seed=2957, scale=0.1), HEADS, D, D ** -0.5)
    relp = pack_win_rel(rnd(HEADS, (2 * WS - 1) ** 2, dev=dev, seed=2958, scale=0.5).contiguous(), WS, WS)
    n2 = ((rnd(C, dev=dev, seed=2959) * 0.1 + 1).contiguous(), (rnd(C, dev=dev, seed=2960) * 0.1).contiguous())
    n1 = ((rnd(C, dev=dev, seed=2961) * 0.3 + 1).contiguous(), (rnd(C, dev=dev, seed=2962) * 0.3).contiguous())                  # gamma1 / beta1
    for v in (*n1, *n2):
        assert v.unique().numel() == C
    return dict(pm=pm, wf=wf, relp=relp, n1=n1, n2=n2)


@pytest.mark.parametrize("H,W,B,shift", [(32, 32, 1, 0), (32, 32, 1, 8), (16, 64, 1, 8), (32, 48, 2, 8)],
                         ids=["32x32-shift0", "32x32-shift8-mask", "16x64-one-window-row", "32x48-B2-two-gates"])
def test_hab_link_equals_the_pair_with_nan_pads(dev, weights, H, W, B, shift):
    w = weights
    with _Bf16Mode() as ops:
        att = _nan_padded(ops, rnd(B, H, W, C, dev=dev, seed=2970), True)
        c2 = _nan_padded(ops, rnd(B, H, W, C, dev=dev, seed=2971), True)
        x = _nan_padded(ops, rnd(B, H, W, C, dev=dev, seed=2972), False)
        gate = (torch.sigmoid(rnd(B, C, dev=dev, seed=2973)) * 0.5 + 0.25).contiguous()      # channel-dependent, one row per image
        assert gate.unique().numel() == B * C
        if B == 1:
            gate = gate.reshape(-1)
        x_ref = ops.token_projmlp(att, x, w["pm"], *w["n2"], c2=c2, c2_scale=gate)
        att_ref = ops.empty_rows_bf16((B, H, W, C), dev)
        _, xn_ref = ops.win_attn_fused(x_ref, att_ref, w["wf"], w["relp"], gamma=w["n1"][0], beta=w["n1"][1], H=H, W=W, Hp=H, Wp=W,
                                       win=(WS, WS), shift=(shift, shift), use_mask=shift > 0, want_xn="bf16")
        x_out, xn, att_out = ops.hab_link(att, x, w["pm"], *w["n2"], c2=c2, c2_scale=gate, wf=w["wf"], rel_padded=w["relp"],
                                          gamma1=w["n1"][0], beta1=w["n1"][1], shift=(shift, shift), use_mask=shift > 0)
        torch.cuda.synchronize()
        for name, got in (("x_out", x_out), ("xn", xn), ("att", att_out)):
            assert torch.isfinite(got.float()).all(), f"{name}: a pad column reached the result"
        assert torch.isfinite(x_ref).all() and torch.isfinite(xn_ref.float()).all() and torch.isfinite(att_ref.float()).all()
        assert torch.equal(x_out, x_ref), f"x_out: max diff {(x_out - x_ref).abs().max().item():.3e}"
        assert torch.equal(xn, xn_ref), f"xn: max diff {(xn.float() - xn_ref.float()).abs().max().item():.3e}"
        assert torch.equal(att_out, att_ref), f"att: max diff {(att_out.float() - att_ref.float()).abs().max().item():.3e}"
        if B == 2:
            assert not torch.equal(x_out[0], x_out[1])


@pytest.mark.parametrize("case", [dict(M=1024, c2=False, io=1), dict(M=1024, c2=True, io=3)], ids=["ocab-form-no-c2", "hab-form-c2-gate"])
def test_token_projmlp_against_the_stage_rounded_reference(dev, case):
    """32 x 32 tokens, four workgroups.  Reference, caps and tolerance are those of tests/test_lowprec_fused_gpu.py."""
    from isr2_amd.prep import pack_token_projmlp
    inp, sr = S.reference("token_projmlp", case)
    S.assert_caps(sr, f"token_projmlp [{S.case_name(case)}]")
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    with _Bf16Mode() as ops:
        d["att"] = _nan_padded(ops, d["att"], True)
        d["x"] = _nan_padded(ops, d["x"], False)
        if case["c2"]:
            d["c2"] = _nan_padded(ops, d["c2"], True)
            assert d["c2_scale"].unique().numel() == C
        out = ops.token_projmlp(d["att"], d["x"], pack_token_projmlp(d["wp"], d["bp"], d["w1"], d["b1"], d["w2"], d["b2"]), d["gamma"], d["beta"],
                                c2=d.get("c2"), c2_scale=d.get("c2_scale"))
    assert out.dtype == torch.float32 and torch.isfinite(out).all()
    err, exc = S.compare(out.contiguous().cpu(), sr)
    print(f"token_projmlp [{S.case_name(case)}]: err = {err:.3e}, err - allow = {exc:.3e}")
    assert exc <= S.FP32_CHAIN_TOL, f"token_projmlp [{S.case_name(case)}]: err - allow = {exc:.3e} > {S.FP32_CHAIN_TOL:.1e}"
