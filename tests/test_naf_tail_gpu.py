"""ff_naf_tail (csrc/naf_tail.hip): the NAFBlock tail in one launch, plain bf16.

The contract is bit-equality with the two launches it replaces -- ops.linear(g, W3, b3, res=x, mul=beta, kmul=sca) followed by
ops.naf_ffn -- and, against an fp64 evaluation of the formula, the bound the existing plain-bf16 check of naf_ffn uses
(tests/test_ops_gpu.py: max|d| <= 3e-2 * max(1, max|ref|))."""
import math

import pytest
import torch
import torch.nn.functional as F

BF16_FFN_TOL = 3e-2


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
    yield
    ops.set_gemm_mode(old)


def rnd(*shape, dev, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def _block(C, dev, seed):
    s = 1.0 / math.sqrt(C)
    return dict(w3=rnd(C, C, dev=dev, seed=seed + 1, scale=s), b3=rnd(C, dev=dev, seed=seed + 2, scale=0.1),
                w4=rnd(2 * C, C, dev=dev, seed=seed + 3, scale=s), b4=rnd(2 * C, dev=dev, seed=seed + 4, scale=0.1),
                w5=rnd(C, C, dev=dev, seed=seed + 5, scale=s), b5=rnd(C, dev=dev, seed=seed + 6, scale=0.1),
                sca=(rnd(C, dev=dev, seed=seed + 7) * 0.3 + 1.0).contiguous(), beta=rnd(C, dev=dev, seed=seed + 8) * 0.4,
                gamma=rnd(C, dev=dev, seed=seed + 9) * 0.3, ln_g=rnd(C, dev=dev, seed=seed + 10) * 0.1 + 1,
                ln_b=rnd(C, dev=dev, seed=seed + 11) * 0.1)


def _chain(g, x, k):
    from isr2_amd import ops
    from isr2_amd.prep import pack_naf_ffn
    y = ops.linear(g, k["w3"], k["b3"], res=x, mul=k["beta"], kmul=k["sca"])
    return ops.naf_ffn(y, pack_naf_ffn(k["w4"], k["b4"], k["w5"], k["b5"]), k["ln_g"], k["ln_b"], k["gamma"])


def _fused(g, x, k):
    from isr2_amd import ops
    from isr2_amd.prep import pack_naf_tail
    pk = pack_naf_tail(k["w3"], k["b3"], k["w4"], k["b4"], k["w5"], k["b5"])
    return ops.naf_tail(g, x, pk, k["sca"], k["beta"], k["ln_g"], k["ln_b"], k["gamma"])


def _ref64(g, x, k):
    d = {n: t.double() for n, t in k.items()}
    C = x.shape[-1]
    y = x.double() + d["beta"] * F.linear(g.double() * d["sca"], d["w3"], d["b3"])
    h = F.linear(F.layer_norm(y, (C,), d["ln_g"], d["ln_b"], 1e-6), d["w4"], d["b4"])
    return y + d["gamma"] * F.linear(h[:, :C] * h[:, C:], d["w5"], d["b5"])


def _check(out, chain, ref, name):
    err = (out.double() - ref).abs().max().item()
    err_chain = (chain.double() - ref).abs().max().item()
    bound = BF16_FFN_TOL * max(1.0, ref.abs().max().item())
    ndiff = int((out != chain).sum().item())
    print(f"{name}: max|fused - fp64| = {err:.3e}, max|chain - fp64| = {err_chain:.3e}, bound {bound:.3e}, "
          f"elements differing from the chain: {ndiff} of {out.numel()}")
    assert torch.equal(out, chain), f"{name}: {ndiff} elements differ from the two-launch chain"
    assert err <= bound, f"{name}: max|d| = {err:.3e} > {bound:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("M", [256, 1000, 65536 + 37, 262144])
@pytest.mark.parametrize("C", [64, 128])
def test_naf_tail_is_bit_equal_to_the_two_launches(dev, bf16_mode, C, M):
    k = _block(C, dev, seed=7000 + C)
    g = rnd(M, C, dev=dev, seed=7100 + C, scale=1.2)
    x = rnd(M, C, dev=dev, seed=7200 + C, scale=1.5) + 0.2
    _check(_fused(g, x, k), _chain(g, x, k), _ref64(g, x, k), f"naf_tail C={C} M={M}")


@pytest.mark.gpu
@pytest.mark.parametrize("C", [64, 128])
def test_naf_tail_takes_row_views(dev, bf16_mode, C):
    """g and x as channel slices of wider buffers (ld > C), 16-byte aligned rows."""
    M = 3000 + 17
    k = _block(C, dev, seed=7300 + C)
    gbuf = rnd(M, C + 32, dev=dev, seed=7400 + C, scale=1.2)
    xbuf = rnd(M, 2 * C, dev=dev, seed=7500 + C, scale=1.5) + 0.2
    g, x = gbuf[:, 16:16 + C], xbuf[:, C:]
    assert g.stride(0) > C and x.stride(0) > C
    _check(_fused(g, x, k), _chain(g, x, k), _ref64(g, x, k), f"naf_tail row views C={C}")


@pytest.mark.gpu
def test_naf_tail_runs_on_a_second_device_of_the_process(dev, bf16_mode):
    """C = 64 takes 69 888 B of dynamic LDS, above the 64 KB default: the limit has to be raised on EVERY device the process launches on.
    One workgroup's rows (128) on device 0, then the same launch on device 1; the two outputs are bit-equal."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    C, M = 64, 128
    outs = []
    for d in (0, 1):
        with torch.cuda.device(d):
            dd = torch.device("cuda", d)
            k = _block(C, dd, seed=7700)
            out = _fused(rnd(M, C, dev=dd, seed=7701, scale=1.2), rnd(M, C, dev=dd, seed=7702, scale=1.5) + 0.2, k)
            torch.cuda.synchronize(d)
            outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
def test_naf_tail_refuses_the_other_modes(dev, mode):
    from isr2_amd import lib, ops
    from isr2_amd.prep import pack_naf_tail
    C, M = 64, 512
    k = _block(C, dev, seed=7600)
    pk = pack_naf_tail(k["w3"], k["b3"], k["w4"], k["b4"], k["w5"], k["b5"])
    g, x = rnd(M, C, dev=dev, seed=7601), rnd(M, C, dev=dev, seed=7602)
    old = ops.gemm_mode()
    ops.set_gemm_mode(mode)
    try:
        with ops.profile() as prof:                      # the wrapper raises before it allocates or launches
            with pytest.raises(lib.FFError):
                ops.naf_tail(g, x, pk, k["sca"], k["beta"], k["ln_g"], k["ln_b"], k["gamma"])
        assert prof.records() == []
    finally:
        ops.set_gemm_mode(old)


def test_pack_naf_tail_fragment_order():
    """Fragment f, lane 32 hh + l31, element j of the image = w[row0 + l31][k0 + 8 hh + j] in the order the kernel walks them."""
    from isr2_amd.prep import pack_naf_tail
    for C in (64, 128):
        w3 = torch.arange(C * C, dtype=torch.float32).reshape(C, C) % 251
        w4 = (torch.arange(2 * C * C, dtype=torch.float32).reshape(2 * C, C) * 3) % 241
        w5 = (torch.arange(C * C, dtype=torch.float32).reshape(C, C) * 7) % 239         # all exactly representable in bf16
        z = torch.zeros(C)
        pk = pack_naf_tail(w3, z, w4, torch.zeros(2 * C), w5, z)
        img = pk["w"].float().reshape(-1, 2, 32, 8)                                      # [fragment][hh][l31][j]
        assert img.shape[0] * 512 == 4 * C * C
        KS, NT = C // 16, C // 32
        pos = torch.arange(32)
        src = (pos & ~12) | ((pos & 4) << 1) | ((pos & 8) >> 1)
        for hh in (0, 1):
            for n in range(NT):
                for st in range(KS):
                    assert torch.equal(img[n * KS + st, hh], w3[32 * n:32 * n + 32, 16 * st + 8 * hh:16 * st + 8 * hh + 8])
            for g in range(NT):
                for half in (0, 1):
                    for st in range(KS):
                        rows = slice(half * C + 32 * g, half * C + 32 * g + 32)
                        assert torch.equal(img[NT * KS + (2 * g + half) * KS + st, hh], w4[rows, 16 * st + 8 * hh:16 * st + 8 * hh + 8])
                for n in range(NT):
                    for s in range(2):
                        cols = 32 * g + src[16 * s + 8 * hh:16 * s + 8 * hh + 8]
                        assert torch.equal(img[3 * NT * KS + (g * NT + n) * 2 + s, hh], w5[32 * n:32 * n + 32][:, cols])


@pytest.mark.gpu
def test_plan_with_naf_tail_exports_and_replays(dev, bf16_mode, tmp_path, synth_sd):
    """A plain-bf16 plan carries ff_naf_tail (the dispatcher is generated from the header) and the C executor replays it bit for bit."""
    import os
    import numpy as np
    from isr2_amd import plan
    from isr2_amd.model import FreqFusionHIP
    model = FreqFusionHIP(synth_sd, dev)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c48_u8.npz"))
    lr = torch.from_numpy(g["lr"]).to(dev)
    stem = str(tmp_path / "ff48_bf16")
    info = plan.export_plan(model, lr, stem)
    assert info["calls"] > 1000
    blob = open(stem + ".ffplan", "rb").read()
    assert b"ff_naf_tail" in blob and b"ff_naf_ffn" not in blob          # both HR levels take the fused tail in this mode
    ref = model(lr)
    nat = plan.NativeModel(stem + ".ffplan", stem + ".ffwts")
    try:
        out = nat(lr)
        torch.cuda.synchronize()
        assert torch.equal(out, ref), "C executor differs from the Python-sequenced forward"
    finally:
        nat.close()
