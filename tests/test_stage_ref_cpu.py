"""CPU checks of tests/golden/stage_ref.py, the stage-rounded fp64 references tests/test_lowprec_fused_gpu.py holds the fused plain-bf16
kernels to.  No GPU: an fp32 stand-in of every kernel's chain -- fp32 LayerNorm and pointwise arithmetic, bf16_rne at the kernel's cast
sites, lowprec_ref.chunked_fp32_matmul for every GEMM -- plays the kernel, over the SAME case table the GPU test runs.

Per kernel and case:
  * the stand-in passes the module's assertion (per element, the fp32 bound plus the allowance);
  * both caps on the allowance hold (stage_ref.assert_caps), computed from the reference alone;
  * the measured noise factors -- GEMM and LayerNorm -- stay within stage_ref's constants (and within their MEASURED values times
    1.25: the constants are supposed to be four times what is measured here, not more);
  * every mutant of the stand-in FAILS the assertion:
        trunc<i>    bf16_trunc instead of bf16_rne at rounding point i (each in turn)
        gelu        the other GELU form (erf <-> tanh)
        scale       a scale applied after the rounding instead of before (naf_tail: sca; token_linear_gated: cm; sgfn_tail: the x1 factor)
        drop        one column of the last GEMM's operand dropped
        swap        two columns of the last GEMM's operand exchanged
        row         the last row of the case computed from its neighbour's input
    A mutant the assertion cannot tell from the stand-in is reported by name (STAGE_REF_UNDETECTED) and fails the test unless it is
    listed in UNDETECTABLE with its reason.  That table is empty: at these shapes every listed mutant is rejected in every case.  Not
    applicable (there is nothing to mutate) and therefore absent from the lists below: `gelu` for the kernels without one (naf_ffn,
    naf_tail, naf_front, sgfn_tail), `scale` for the kernels that scale nothing before a rounding (token_mlp, token_projmlp, naf_ffn,
    naf_front; c2_scale of token_projmlp enters after the projection, in fp32).  trunc0 of token_projmlp on bf16 att rows is not a
    mutant either (the rows are exact operands), so it runs on the fp32-att cases only.  All scales are non-powers of two (a power of two
    commutes with the rounding)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import lowprec_ref as R  # noqa: E402
import stage_ref as S  # noqa: E402

UNDETECTABLE = {}             # (kernel, mutant) -> why the assertion cannot see it


class Arith:
    """The stand-in's arithmetic, with at most one mutation switched on."""

    def __init__(self, mut=None):
        self.mut, self.rp, self.applied = mut, 0, mut is None

    def round(self, x):
        """A rounding point (numbered in the order the chain reaches them)."""
        i, self.rp = self.rp, self.rp + 1
        if self.mut == f"trunc{i}":
            self.applied = True
            return R.bf16_trunc(x)
        return R.bf16_rne(x)

    def mm(self, a, w, b=None):
        y = R.chunked_fp32_matmul(a, R.bf16_rne(w))
        return y if b is None else y + b

    def last_operand(self, a):
        """The (rounded) operand of the chain's last GEMM: where the column mutants act."""
        if self.mut == "drop":
            self.applied = True
            a = a.clone()
            a[:, 5] = 0.0
        elif self.mut == "swap":
            self.applied = True
            a = a.clone()
            a[:, [3, 40]] = a[:, [40, 3]]
        return a

    def gelu(self, x, form):
        if self.mut == "gelu":
            self.applied = True
            form = "tanh" if form == "erf" else "erf"
        return F.gelu(x, approximate="tanh") if form == "tanh" else F.gelu(x)

    def rows(self, x):
        """A row-wise input: the `row` mutant computes the last row from its neighbour's."""
        if self.mut == "row":
            self.applied = True
            x = x.clone()
            x[-1] = x[-2]
        return x

    def scale_after(self):
        if self.mut == "scale":
            self.applied = True
            return True
        return False


def ln32(x, g, b, eps):
    return S.layernorm_fp32(x, g, b, eps)


def token_mlp_standin(A, x, gamma, beta, w1, b1, w2, b2, eps=1e-5):
    a1 = A.round(ln32(A.rows(x), gamma, beta, eps))
    a2 = A.last_operand(A.round(A.gelu(A.mm(a1, w1, b1), "erf")))
    return x + b2 + A.mm(a2, w2)


def token_projmlp_standin(A, att, x, wp, bp, w1, b1, w2, b2, gamma, beta, c2=None, c2_scale=None, eps=1e-5):
    a0 = A.rows(att.float()) if att.dtype == torch.bfloat16 else A.round(A.rows(att))
    if att.dtype == torch.bfloat16:
        A.rp += 1                                           # keep the numbering: rounding point 0 is att's
    x1 = A.mm(a0, wp, bp) + (x if c2 is None else x + c2.float() * c2_scale)
    a1 = A.round(ln32(x1, gamma, beta, eps))
    a2 = A.last_operand(A.round(A.gelu(A.mm(a1, w1, b1), "tanh")))
    return x1 + A.mm(a2, w2) + b2


def token_linear_gated_standin(A, x, x2, cm, gw1, gb1, gw2, gb2, w, b, res=None):
    xs = A.rows(x)
    ga = A.gelu(A.mm(A.round(xs), gw1, gb1), "erf")
    sm = torch.sigmoid(ga.matmul(gw2.reshape(-1, 1)) + gb2)
    if A.scale_after():
        mix = A.round(R.bf16_rne(xs) * cm + x2 * sm)       # cm applied to the ROUNDED x
        A.rp -= 1
    else:
        mix = xs * cm + x2 * sm
    o = A.mm(A.last_operand(A.round(mix)), w, b)
    return o if res is None else o + res


def _naf_ffn_standin(A, y, w4, b4, w5, b5, ln_g, ln_b, oscale, eps):
    C = y.shape[-1]
    h = A.mm(A.round(ln32(y, ln_g, ln_b, eps)), w4, b4)
    a2 = A.last_operand(A.round(h[:, :C] * h[:, C:]))
    return (A.mm(a2, w5) + b5) * oscale + y


def naf_ffn_standin(A, y, w4, b4, w5, b5, ln_g, ln_b, oscale, eps=1e-6):
    return _naf_ffn_standin(A, A.rows(y), w4, b4, w5, b5, ln_g, ln_b, oscale, eps) + (y - A.rows(y))     # (the `row` mutant keeps the true residual)


def naf_tail_standin(A, g, x, w3, b3, w4, b4, w5, b5, sca, beta, ln_g, ln_b, gamma, eps=1e-6):
    gs = A.rows(g)
    a0 = A.round(gs) * sca if A.scale_after() else A.round(gs * sca)
    y = (A.mm(a0, w3) + b3) * beta + x
    return _naf_ffn_standin(A, y, w4, b4, w5, b5, ln_g, ln_b, gamma, eps)


def naf_front_standin(A, x, w1, b1, ln_g, ln_b, wdw, bdw, eps=1e-6):
    _, H, W, C = x.shape
    a1 = A.last_operand(A.round(ln32(A.rows(x.reshape(H * W, C)), ln_g, ln_b, eps)))
    t = A.mm(a1, w1, b1).reshape(1, H, W, 2 * C).permute(0, 3, 1, 2)
    d = F.conv2d(t, wdw, bdw, padding=1, groups=2 * C).permute(0, 2, 3, 1)
    gate = d[..., :C] * d[..., C:]
    return gate, gate.mean(dim=(1, 2))


def sgfn_tail_standin(A, y, c2, wd, bd, stats, gamma, beta, w2, b2, res=None):
    _, H, W, _ = y.shape
    ys = A.rows(y.reshape(H * W, -1)).reshape(1, H, W, -1)
    x1, x2 = ys[..., :c2], ys[..., c2:2 * c2]
    st = stats.reshape(1, H, W, 2)
    xn = (x2 - st[..., 0:1]) * st[..., 1:2] * gamma + beta
    conv = F.conv2d(xn.permute(0, 3, 1, 2), wd, bd, padding=1, groups=c2).permute(0, 2, 3, 1)
    if A.scale_after():
        gate = A.round(R.bf16_rne(conv) * x1)                # x1 applied to the ROUNDED convolution
        A.rp -= 1
    else:
        gate = conv * x1
    o = A.mm(A.last_operand(A.round(gate.reshape(H * W, c2))), w2, b2).reshape(1, H, W, -1)
    return o if res is None else o + res


STANDINS = dict(token_mlp=token_mlp_standin, token_projmlp=token_projmlp_standin, token_linear_gated=token_linear_gated_standin,
                naf_ffn=naf_ffn_standin, naf_tail=naf_tail_standin, naf_front=naf_front_standin, sgfn_tail=sgfn_tail_standin)
COLS = ["drop", "swap", "row"]
MUTANTS = dict(token_mlp=["trunc0", "trunc1", "gelu"] + COLS,
               token_projmlp=["trunc0", "trunc1", "trunc2", "gelu"] + COLS,
               token_linear_gated=["trunc0", "trunc1", "gelu", "scale"] + COLS,
               naf_ffn=["trunc0", "trunc1"] + COLS,
               naf_tail=["trunc0", "trunc1", "trunc2", "scale"] + COLS,
               naf_front=["trunc0"] + COLS,
               sgfn_tail=["trunc0", "scale"] + COLS)
ALL = [(k, c) for k, cases in S.CASES.items() for c in cases]
NOISE = {}                    # kernel -> [largest GEMM ratio, largest LayerNorm ratio] measured in this run


@pytest.fixture(scope="module")
def noise_report():
    yield
    print("\nSTAGE_REF_NOISE " + " ".join(f"{k}: gemm {v[0]:.2f} ln {v[1]:.2f};" for k, v in sorted(NOISE.items()))
          + f" constants: gemm {S.GEMM_NOISE_MEASURED} x {S.GEMM_NOISE_FACTOR}, ln {S.LN_NOISE_MEASURED} x {S.GEMM_NOISE_FACTOR}")


def _refs(sr):
    return (sr,) if isinstance(sr, S.StageRef) else tuple(sr)


def _outs(out):
    return out if isinstance(out, tuple) else (out,)


def _excess(out, sr):
    """Worst excess over the kernel's outputs (naf_front has two)."""
    return max(S.compare(o, r)[1] for o, r in zip(_outs(out), _refs(sr)))


@pytest.mark.parametrize("kernel,case", ALL, ids=[f"{k}-{S.case_name(c)}" for k, c in ALL])
def test_standin_passes_mutants_fail_and_caps_hold(kernel, case, noise_report):
    inp, sr = S.reference(kernel, case)
    name = f"{kernel} [{S.case_name(case)}]"
    # the two caps, from the reference alone, before any output is looked at
    for i, r in enumerate(_refs(sr)):
        S.assert_caps(r, name + (" pooled" if i else ""))
    # the noise factors
    first = _refs(sr)[0]
    g = max(S.gemm_noise_ratio(*o) for o in first.gemms)
    ln = max((S.ln_noise_ratio(*o) for o in first.lns), default=0.0)
    n = NOISE.setdefault(kernel, [0.0, 0.0])
    n[0], n[1] = max(n[0], g), max(n[1], ln)
    print(f"STAGE_REF_NOISE {name}: gemm {g:.3f} (constant {S.GEMM_NOISE_C:.1f}), LayerNorm {ln:.3f} (constant {S.LN_NOISE_C:.1f})")
    assert g <= S.GEMM_NOISE_C and g <= 1.25 * S.GEMM_NOISE_MEASURED, (g, S.GEMM_NOISE_MEASURED)
    assert ln <= S.LN_NOISE_C and ln <= 1.25 * S.LN_NOISE_MEASURED, (ln, S.LN_NOISE_MEASURED)
    # the stand-in
    A = Arith()
    out = STANDINS[kernel](A, **inp)
    err = max(S.compare(o, r)[0] for o, r in zip(_outs(out), _refs(sr)))
    exc = _excess(out, sr)
    print(f"STAGE_REF_STANDIN {name}: err {err:.3e}, err - allow {exc:.3e} of max(1, max|ref|) (bound {S.FP32_CHAIN_TOL:.0e})")
    assert exc <= S.FP32_CHAIN_TOL, f"{name}: the fp32 stand-in is outside the bound by {exc:.3e}"
    # the mutants
    undetected = []
    for mut in MUTANTS[kernel]:
        if kernel == "token_projmlp" and mut == "trunc0" and case["io"] & 1:
            continue                                        # bf16 att rows are exact operands: nothing is rounded there
        A = Arith(mut)
        bad = STANDINS[kernel](A, **inp)
        assert A.applied, f"{name}: mutant {mut} was never applied"
        e = _excess(bad, sr)
        print(f"STAGE_REF_MUTANT {name} {mut}: err - allow {e:.3e} ({e / S.FP32_CHAIN_TOL:.1f} x the bound)")
        if e <= S.FP32_CHAIN_TOL:
            print(f"STAGE_REF_UNDETECTED {name} {mut}: {UNDETECTABLE.get((kernel, mut), 'NOT LISTED')}")
            if (kernel, mut) not in UNDETECTABLE:
                undetected.append(mut)
    assert not undetected, f"{name}: mutants the assertion did not reject: {undetected}"


def test_round_point_and_branching():
    """round_point flags exactly the elements whose rounding a delta can change, and branch_round_point's variants are those two
    values (variant 0 the nominal one)."""
    v = torch.tensor([[1.0, 1.00390625, 0.5019531, 1.0039, 0.3, -2.0078125, 5.0, 1e-3]], dtype=torch.float64)   # 1 + 2^-8 is a tie of [1, 2)
    d = torch.full_like(v, 1e-6)
    a, mv = S.round_point(v, d)
    assert torch.equal(a, R.bf16_rne(v.float()).double())
    assert mv[0].gt(0).tolist() == [False, True, True, False, False, True, False, False]
    assert mv[0, 1].item() == 2.0 ** -7 and mv[0, 5].item() == 2.0 ** -6
    av, mvv, ri = S.branch_round_point(v, d, nb=2)
    assert av.shape == (4, 8) and ri.tolist() == [0, 0, 0, 0] and torch.equal(av[0], a[0])
    # the two largest movers (indices 5 and 1) are enumerated, the third (index 2) is left to propagation in every variant
    assert sorted({(r[5].item(), r[1].item()) for r in av}) == [(-2.015625, 1.0), (-2.015625, 1.0078125), (-2.0, 1.0), (-2.0, 1.0078125)]
    assert (mvv[:, [1, 5]] == 0).all() and (mvv[:, 2] == 2.0 ** -8).all()
    assert all(torch.equal(r[[0, 2, 3, 4, 6, 7]], a[0, [0, 2, 3, 4, 6, 7]]) for r in av)


def test_references_match_plain_fp64_formulas():
    """Each stage-rounded reference against the UNROUNDED fp64 formula written with torch's own layers: they differ by the operand
    rounding only (about 2^-8 per operand, a few 1e-3 of max|ref| at the output) -- a wrong formula would be far outside."""
    for kernel, case in ((k, cs[0]) for k, cs in S.CASES.items()):
        inp, sr = S.reference(kernel, case)
        d = {k: (v.double() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
        if kernel == "token_mlp":
            x = d["x"]
            plain = x + F.linear(F.gelu(F.linear(F.layer_norm(x, x.shape[-1:], d["gamma"], d["beta"], 1e-5), d["w1"], d["b1"])), d["w2"], d["b2"])
        elif kernel == "token_projmlp":
            x1 = d["x"] + F.linear(d["att"], d["wp"], d["bp"])
            plain = x1 + F.linear(F.gelu(F.linear(F.layer_norm(x1, x1.shape[-1:], d["gamma"], d["beta"], 1e-5), d["w1"], d["b1"])), d["w2"], d["b2"])
        elif kernel == "token_linear_gated":
            sm = torch.sigmoid(F.linear(F.gelu(F.linear(d["x"], d["gw1"], d["gb1"])), d["gw2"]) + d["gb2"])
            plain = d["res"] + F.linear(d["x"] * d["cm"] + d["x2"] * sm, d["w"], d["b"])
        elif kernel in ("naf_ffn", "naf_tail"):
            C = case["C"]
            y = d["y"] if kernel == "naf_ffn" else d["x"] + d["beta"] * F.linear(d["g"] * d["sca"], d["w3"], d["b3"])
            h = F.linear(F.layer_norm(y, (C,), d["ln_g"], d["ln_b"], 1e-6), d["w4"], d["b4"])
            plain = y + (d["oscale"] if kernel == "naf_ffn" else d["gamma"]) * F.linear(h[:, :C] * h[:, C:], d["w5"], d["b5"])
        elif kernel == "naf_front":
            C = case["C"]
            t = F.linear(F.layer_norm(d["x"], (C,), d["ln_g"], d["ln_b"], 1e-6), d["w1"], d["b1"]).permute(0, 3, 1, 2)
            t = F.conv2d(t, d["wdw"], d["bdw"], padding=1, groups=2 * C).permute(0, 2, 3, 1)
            plain = t[..., :C] * t[..., C:]
            sr = sr[0]
        else:
            c2 = d["c2"]
            x2n = F.layer_norm(d["y"][..., c2:], (c2,), d["gamma"], d["beta"], 1e-5).permute(0, 3, 1, 2)
            gate = d["y"][..., :c2] * F.conv2d(x2n, d["wd"], d["bd"], padding=1, groups=c2).permute(0, 2, 3, 1)
            plain = d["res"] + F.linear(gate, d["w2"], d["b2"])
        err = R.rel_err(plain.reshape(sr.ref[0].shape), sr.ref[0])
        print(f"{kernel}: stage-rounded vs unrounded fp64 formula: {err:.3e} of max(1, max|ref|)")
        assert 1e-5 < err < 2e-2, (kernel, err)
