"""ff_gemm_rows_bf16 (csrc/gemm_rows_bf16.hip) and the bf16-rows route of NAFNet's deep blocks, plain bf16.

The contract is bit-equality with what it replaces: ff_conv2d_bf16s(nterms = 1) on the fp32 upcast of the same bf16 rows (the upcast is
exact, so the old kernel's staging cast returns the same bf16), ff_layernorm followed by a bf16 cast, and the whole NAFNet forward with
the route off.  Against the operand-rounded fp64 reference (tests/golden/lowprec_ref.py) the kernel is held to the bound of
tests/test_lowprec_exact_gpu.py: 2e-5 of max(1, max|ref|), plus half a bf16 ulp where the output is stored as bf16.

Every buffer a kernel writes is allocated with a NaN guard band (rows before and after, and the columns between N and the pitch) that
must stay untouched; every buffer it reads is surrounded by 1e30, so an over-read shows up as a wrong result, never as a fault."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from lowprec_ref import FP32_CHAIN_TOL as TOL  # noqa: E402

G = 3            # guard rows on either side of every buffer
BIG = 1e30


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isr2_amd import lib
    lib.load()
    return torch.device("cuda:0")


@pytest.fixture
def bf16_mode(dev):
    from isr2_amd import ops
    old = ops.gemm_mode()
    ops.set_gemm_mode("bf16")
    yield ops
    ops.set_rows_gemm(True)
    ops.set_gemm_mode(old)


def rnd(*shape, dev, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def _cases():
    """(M, N, K, epilogue, bias, mul, lda - K, ldo - channels, ldr - N, tile_hint); epilogue: plain = bias -> fp32 rows, gate = SimpleGate
    pair product -> bf16 rows, res = bias, mul, residual -> fp32 rows, kmul = fp32 A rows scaled per input channel, then as res."""
    c = []
    for hint in (1, 2):                             # every tile form x every epilogue, ragged in M and N, odd chunk count, all pitches padded
        for epi in ("plain", "gate", "res", "kmul"):
            c.append((129, 136, 192, epi, True, epi == "res", 64, 8, 12, hint))
    for M in (1, 127, 128, 129, 4096 + 37):         # M: below / at / above one tile, ragged last tile of many
        c.append((M, 128, 128, "plain", True, False, 0, 0, 0, 0))
        c.append((M, 136, 64, "gate", True, False, 8, 4, 0, 0))
        c.append((M, 64, 128, "res", False, True, 0, 4, 8, 0))
        c.append((M, 136, 192, "kmul", True, True, 4, 0, 4, 0))
    for N in (64, 128, 136, 2048):
        c.append((300, N, 192, "res", True, False, 64, 0, 4, 0))
    for K in (64, 128, 192, 1024):                  # one chunk (prologue = epilogue), even / odd chunk counts, long
        c.append((257, 256, K, "gate", False, False, 0, 0, 0, 0))
        c.append((257, 128, K, "plain", False, False, 8, 0, 0, 0))
    c.append((4096 + 37, 2048, 1024, "plain", True, False, 0, 0, 0, 0))      # more than 256 tiles: the automatic rule takes 128 x 128
    c.append((4096 + 37, 2048, 1024, "gate", True, False, 0, 0, 0, 1))
    c.append((4096 + 37, 2048, 1024, "res", True, True, 0, 0, 0, 2))
    c.append((4096 + 37, 1024, 1024, "kmul", True, True, 0, 0, 0, 0))
    c.append((300, 128, 64, "kmul", False, False, 0, 0, 0, 0))
    return c


CASES = _cases()
IDS = [f"M{m}-N{n}-K{k}-{e}-b{int(b)}m{int(mu)}-p{pa}.{po}.{pr}-t{h}" for m, n, k, e, b, mu, pa, po, pr, h in CASES]


def _guarded(rows, cols, ld, dev, dtype, fill, data=None):
    """[rows + 2 G][ld] filled with `fill`; returns (buffer, view of rows x cols in its middle), the view holding `data` if given."""
    buf = torch.full((rows + 2 * G, ld), fill, device=dev, dtype=dtype)
    view = buf[G:G + rows, :cols]
    if data is not None:
        view.copy_(data)
    return buf, view


def _guard_untouched(buf, rows, cols):
    """Everything outside the rows x cols view is still NaN, everything inside is finite."""
    nan = torch.isnan(buf.float())
    inside = nan[G:G + rows, :cols]
    return int(nan.sum().item()) == buf.numel() - rows * cols and not bool(inside.any().item())


def _setup(case, dev, ops):
    import lowprec_ref as R
    M, N, K, epi, has_b, has_m, pa, po, pr, hint = case
    seed = 9000 + 7 * M + 3 * N + K
    gate = epi == "gate"
    No = N // 2 if gate else N
    a32in = epi == "kmul"                                                      # fp32 A rows (not pre-rounded) with the fp32 channel scale
    x = rnd(M, K, dev=dev, seed=seed)
    x = x if a32in else R.bf16_rne(x)                                          # bf16 values held in fp32
    kmul = (rnd(K, dev=dev, seed=seed + 5) * 0.3 + 1.0).contiguous() if a32in else None
    w = rnd(N, K, dev=dev, seed=seed + 1, scale=1.0 / math.sqrt(K))
    bias = rnd(N, dev=dev, seed=seed + 2, scale=0.1) if has_b else None
    mul = rnd(N, dev=dev, seed=seed + 3) if has_m else None
    res = rnd(M, N, dev=dev, seed=seed + 4) if epi in ("res", "kmul") else None
    hi = ops._split_weight(w, True, K)[0]
    assert tuple(hi.shape) == (N, K)
    _, a16 = _guarded(M, K, K + pa, dev, torch.bfloat16, BIG, x) if not a32in else (None, None)
    _, a32 = _guarded(M, K, K + pa, dev, torch.float32, BIG, x)
    _, wv = _guarded(N, K, K, dev, torch.bfloat16, BIG, hi)
    rv = _guarded(M, N, N + pr, dev, torch.float32, BIG, res)[1] if res is not None else None
    return dict(M=M, N=N, K=K, gate=gate, No=No, hint=hint, x=x, w=w, bias=bias, mul=mul, res=res, a16=a16, a32=a32, wv=wv, rv=rv,
                ldo=No + po, kmul=kmul)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _run_new(s, dev):
    from isr2_amd import lib
    L = lib.load()
    buf, out = _guarded(s["M"], s["No"], s["ldo"], dev, torch.bfloat16 if s["gate"] else torch.float32, float("nan"))
    st = torch.cuda.current_stream().cuda_stream
    a = s["a32"] if s["a16"] is None else s["a16"]
    lib.check(L.ff_gemm_rows_bf16(a.data_ptr(), 1 if s["a16"] is None else 0, a.stride(0), s["wv"].data_ptr(), s["K"], _ptr(s["kmul"]), _ptr(s["bias"]), _ptr(s["mul"]),
                                  _ptr(s["rv"]), s["rv"].stride(0) if s["rv"] is not None else 0, out.data_ptr(), s["ldo"], s["M"], s["N"],
                                  s["K"], 1 if s["gate"] else 0, s["hint"], st))
    return buf, out


def _run_old(s, dev):
    from isr2_amd import lib
    L = lib.load()
    buf, out = _guarded(s["M"], s["No"], s["ldo"], dev, torch.float32, float("nan"))
    st = torch.cuda.current_stream().cuda_stream
    K, M, N = s["K"], s["M"], s["N"]
    lib.check(L.ff_conv2d_bf16s(s["a32"].data_ptr(), s["wv"].data_ptr(), None, K, K, _ptr(s["bias"]), _ptr(s["mul"]), _ptr(s["rv"]),
                                out.data_ptr(), 1, 1, M, K, s["a32"].stride(0), 1, M, N, s["ldo"], s["rv"].stride(0) if s["rv"] is not None else 0,
                                1, 1, 1, 1, 0, 0, 0, 1.0, 1 if s["gate"] else 0, 1, 0, _ptr(s["kmul"]), st))
    return buf, out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_gemm_is_bit_equal_to_the_fp32_rows_kernel(dev, bf16_mode, case):
    s = _setup(case, dev, bf16_mode)
    nbuf, new = _run_new(s, dev)
    obuf, old = _run_old(s, dev)
    torch.cuda.synchronize()
    assert _guard_untouched(obuf, s["M"], s["No"]), "the reference kernel wrote outside M x N"
    assert _guard_untouched(nbuf, s["M"], s["No"]), "ff_gemm_rows_bf16 wrote outside M x N (or left NaN inside)"
    want = old.to(torch.bfloat16) if s["gate"] else old
    ndiff = int((new != want).sum().item())
    print(f"rows gemm {case}: elements differing from ff_conv2d_bf16s: {ndiff} of {new.numel()}")
    assert new.dtype == want.dtype and torch.equal(new, want), f"{ndiff} elements differ"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_gemm_against_the_fp64_reference(dev, bf16_mode, case):
    import lowprec_ref as R
    s = _setup(case, dev, bf16_mode)
    _, new = _run_new(s, dev)
    ref = R.epilogue_f64(R.operand_a(s["x"], "bf16", s["kmul"]).matmul(R.operand_w(s["w"]).t()), s["bias"], None, s["mul"], 1.0, s["res"], gate_pairs=s["gate"])
    err = R.rel_err(new.float(), ref)
    if s["gate"]:                                    # stored as bf16: half a bf16 ulp on top of the fp32-chain bound
        excess = R.bf16_row_excess(new.float(), ref)
        print(f"rows gemm {case}: err = {err:.3e}, excess over 2^-8 |ref| + {TOL:.0e} max(1, max|ref|) = {excess:.3e}")
        assert excess <= 0.0
    else:
        print(f"rows gemm {case}: err = {err:.3e} of max(1, max|ref| = {ref.abs().max().item():.3e})")
        assert err <= TOL


def test_rows_gemm_refuses_what_it_cannot_take(dev, bf16_mode):
    """Route conditions are checked in the launcher: a refused call launches nothing."""
    from isr2_amd import lib
    L = lib.load()
    a = torch.zeros(64, 128, device=dev, dtype=torch.bfloat16)
    w = torch.zeros(64, 128, device=dev, dtype=torch.bfloat16)
    out = torch.full((64, 64), float("nan"), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    bad = [dict(K=96, Kp=96), dict(K=64, Kp=128), dict(lda=132), dict(ldo=66), dict(gate=2), dict(hint=9), dict(aoff=2), dict(kmul=w.data_ptr()),
           dict(a32=1, gate=1), dict(a32=2)]
    for b in bad:
        K = b.get("K", 128)
        rc = L.ff_gemm_rows_bf16(a.data_ptr() + b.get("aoff", 0), b.get("a32", 0), b.get("lda", 128), w.data_ptr(), b.get("Kp", K), b.get("kmul"), None, None, None, 0,
                                 out.data_ptr(), b.get("ldo", 64), 64, 64, K, b.get("gate", 0), b.get("hint", 0), st)
        assert rc != 0, b
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all().item())
    x = torch.zeros(8, 128, device=dev, dtype=torch.bfloat16)
    wf = torch.zeros(64, 128, device=dev)
    for mode in ("bf16x3", "f32"):                   # bf16 rows exist in plain-bf16 mode only
        bf16_mode.set_gemm_mode(mode)
        with pytest.raises(lib.FFError):
            bf16_mode.linear(x, wf)
    bf16_mode.set_gemm_mode("bf16")
    with pytest.raises(lib.FFError):                 # the channel scale is an fp32 multiply: fp32 rows only
        bf16_mode.linear(x, wf, kmul=torch.ones(128, device=dev))


@pytest.mark.parametrize("rows", [1, 5, 4099])
@pytest.mark.parametrize("C", [256, 320, 1024])
def test_layernorm_bf16out_is_the_rounded_fp32_result(dev, bf16_mode, C, rows):
    ops = bf16_mode
    x = rnd(rows, C, dev=dev, seed=100 + C + rows, scale=1.5) + 0.3
    g = rnd(C, dev=dev, seed=101 + C) * 0.1 + 1
    b = rnd(C, dev=dev, seed=102 + C) * 0.1
    want = ops.layernorm(x, g, b, eps=1e-6).to(torch.bfloat16)
    ld = (C + 63) // 64 * 64 + 64
    buf, out = _guarded(rows, C, ld, dev, torch.bfloat16, float("nan"))
    got = ops.layernorm(x, g, b, eps=1e-6, out=out, out_bf16=True)
    torch.cuda.synchronize()
    assert _guard_untouched(buf, rows, C)
    assert got.dtype == torch.bfloat16 and torch.equal(got, want)
    auto = ops.layernorm(x, g, b, eps=1e-6, out_bf16=True)          # the wrapper's own buffer: pitch a multiple of 64 elements
    assert auto.stride(-2) % 64 == 0 and torch.equal(auto, want)


def test_linear_takes_bf16_rows(dev, bf16_mode):
    """ops.linear routes on the dtype of x: LayerNorm -> bf16 -> conv4 (gated, bf16 out) -> conv5, against the fp32-rows chain."""
    ops = bf16_mode
    M, c = 1000, 256
    y = rnd(1, 25, 40, c, dev=dev, seed=1)
    g, b = rnd(c, dev=dev, seed=2) * 0.1 + 1, rnd(c, dev=dev, seed=3) * 0.1
    w4, b4 = rnd(2 * c, c, dev=dev, seed=4, scale=1 / 16), rnd(2 * c, dev=dev, seed=5, scale=0.1)
    w5, b5, gam = rnd(c, c, dev=dev, seed=6, scale=1 / 16), rnd(c, dev=dev, seed=7, scale=0.1), rnd(c, dev=dev, seed=8)
    old = ops.linear(ops.linear(ops.layernorm(y, g, b, eps=1e-6), w4, b4, gate_pairs=True), w5, b5, res=y, mul=gam)
    sca = (rnd(c, dev=dev, seed=9) * 0.3 + 1.0).contiguous()
    assert torch.equal(ops.linear(y, w5, b5, res=y, mul=gam, kmul=sca, rows_gemm=True), ops.linear(y, w5, b5, res=y, mul=gam, kmul=sca))
    with ops.profile() as prof:
        h = ops.linear(ops.layernorm(y, g, b, eps=1e-6, out_bf16=True), w4, b4, gate_pairs=True, out_bf16=True)
        new = ops.linear(h, w5, b5, res=y, mul=gam)
    assert h.dtype == torch.bfloat16 and new.dtype == torch.float32 and torch.equal(new, old)
    rec = {n: (f, nb) for n, _, f, nb in prof.records()}
    assert set(rec) == {"layernorm", "linear"}                       # accounted under the names bench.py --full's roofline counts
    assert rec["linear"] == (2.0 * M * c * c, 2.0 * (M * c + c * c) + 4.0 * M * c + 4.0 * M * c)   # bytes actually moved: 2 per bf16 element


@pytest.mark.parametrize("hw", [(64, 64), (40, 52)])
def test_nafnet_forward_is_unchanged_by_the_route(dev, bf16_mode, synth_sd, hw):
    from isr2_amd.experts import NafnetHIP
    ops = bf16_mode
    net = NafnetHIP(synth_sd, dev)
    lr = rnd(1, 3, *hw, dev=dev, seed=11).abs().clamp(0, 1)
    outs = {}
    for on in (False, True):
        ops.set_rows_gemm(on)
        taps = {}
        with ops.profile() as prof:
            sr = net.forward(lr, taps=taps)
        names = [r[0] for r in prof.records()]
        outs[on] = (sr.clone(), taps["naf.mid"].clone(), names.count("linear"), names.count("layernorm"))
    assert outs[True][2:] == outs[False][2:]                           # the same launches under the same names
    assert torch.equal(outs[True][1], outs[False][1]), "naf.mid differs between the routes"
    assert torch.equal(outs[True][0], outs[False][0]), "the output differs between the routes"


def test_plan_with_rows_gemm_exports_and_replays(dev, bf16_mode, tmp_path, synth_sd):
    """The new entry points are in the plan with the route on and absent with it off (the dispatcher is generated from the header), and
    the C executor replays the plan bit for bit."""
    import numpy as np
    from isr2_amd import plan
    from isr2_amd.model import FreqFusionHIP
    ops = bf16_mode
    model = FreqFusionHIP(synth_sd, dev)
    lr = torch.from_numpy(np.load(os.path.join(HERE, "golden", "c48_u8.npz"))["lr"]).to(dev)
    ops.set_rows_gemm(False)
    stem_off = str(tmp_path / "ff48_rows_off")
    plan.export_plan(model, lr, stem_off)
    blob = open(stem_off + ".ffplan", "rb").read()
    assert b"ff_gemm_rows_bf16" not in blob and b"ff_layernorm_bf16out" not in blob
    ref_off = model(lr).clone()
    ops.set_rows_gemm(True)
    stem = str(tmp_path / "ff48_rows_on")
    plan.export_plan(model, lr, stem)
    blob = open(stem + ".ffplan", "rb").read()
    assert b"ff_gemm_rows_bf16" in blob and b"ff_layernorm_bf16out" in blob
    ref = model(lr)
    assert torch.equal(ref, ref_off)
    nat = plan.NativeModel(stem + ".ffplan", stem + ".ffwts")
    try:
        out = nat(lr)
        torch.cuda.synchronize()
        assert torch.equal(out, ref), "C executor differs from the Python-sequenced forward"
    finally:
        nat.close()
