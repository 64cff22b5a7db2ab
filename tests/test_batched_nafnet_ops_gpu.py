"""The per-image forms of NAFNet's kernels: naf_front, dwconv3_gate_pool, naf_tail and the two conv3 GEMMs (kmul [B,K]) on a batch of B
images in ONE launch against B single-image calls.  torch.equal throughout: the contract is that every image comes out with the bits of
its own B == 1 call.  Every test also asserts that two images' results differ, so none can pass by broadcasting image 0."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = ["bf16x3", "bf16"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isr2_amd import lib
    lib.load()
    return torch.device("cuda:0")


@pytest.fixture(params=MODES)
def mode(request, dev):
    from isr2_amd import ops
    prev = ops.gemm_mode()
    ops.set_gemm_mode(request.param)
    yield request.param
    ops.set_gemm_mode(prev)


@pytest.fixture
def bf16_mode(dev):
    from isr2_amd import ops
    prev = ops.gemm_mode()
    ops.set_gemm_mode("bf16")
    yield
    ops.set_gemm_mode(prev)


def rnd(*shape, dev, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def _dw(C2, dev, seed):
    """Depth-wise 3x3 weights tap-major [9, 2C] and bias [2C]."""
    return rnd(9, C2, dev=dev, seed=seed, scale=0.3).contiguous(), rnd(C2, dev=dev, seed=seed + 1, scale=0.1)


# 20 x 40 pixels = 2.5 x 2.5 tiles of 8 x 16: partial tiles on both edges, nine partial rows per image
@pytest.mark.parametrize("C", [64, 128])
def test_naf_front_batch_equals_single_calls(dev, mode, C):
    from isr2_amd import ops
    from isr2_amd.prep import pack_token_linear
    B, H, W = 3, 20, 40
    x = rnd(B, H, W, C, dev=dev, seed=100 + C, scale=1.3) + 0.1
    pk = pack_token_linear(rnd(2 * C, C, dev=dev, seed=101 + C, scale=1.0 / math.sqrt(C)), rnd(2 * C, dev=dev, seed=102 + C, scale=0.1))
    ln_g, ln_b = rnd(C, dev=dev, seed=103 + C) * 0.1 + 1, rnd(C, dev=dev, seed=104 + C) * 0.1
    w_tap, dw_b = _dw(2 * C, dev, 105 + C)
    out, pooled = ops.naf_front(x, pk, ln_g, ln_b, w_tap, dw_b)
    assert tuple(out.shape) == (B, H, W, C) and tuple(pooled.shape) == (B, C)
    for b in range(B):
        o1, p1 = ops.naf_front(x[b:b + 1], pk, ln_g, ln_b, w_tap, dw_b)
        assert torch.equal(out[b:b + 1], o1), f"image {b}: out"
        assert torch.equal(pooled[b:b + 1], p1), f"image {b}: pooled"
    assert not torch.equal(out[0], out[1]) and not torch.equal(pooled[0], pooled[1])


# [3,6,8,512]: small, c = 256; [2,2,2,2048]: c = 1024, one item per thread row; [2,18,1024,512]: 5 strips x 1024 columns = 5120 items at
# 4 per workgroup = 1280 > the 1024 cap: the grid-stride second pass, and the last strip is partial
@pytest.mark.parametrize("B,H,W,C2", [(3, 6, 8, 512), (2, 2, 2, 2048), (2, 18, 1024, 512)])
def test_dwconv3_gate_pool_batch_equals_single_calls(dev, B, H, W, C2):
    from isr2_amd import ops
    t = rnd(B, H, W, C2, dev=dev, seed=200 + H)
    w_tap, dw_b = _dw(C2, dev, 201 + H)
    out, pooled = ops.dwconv3_gate_pool(t, w_tap, dw_b)
    assert tuple(out.shape) == (B, H, W, C2 // 2) and tuple(pooled.shape) == (B, C2 // 2)
    for b in range(B):
        o1, p1 = ops.dwconv3_gate_pool(t[b:b + 1], w_tap, dw_b)
        assert torch.equal(out[b:b + 1], o1), f"image {b}: out"
        assert torch.equal(pooled[b:b + 1], p1), f"image {b}: pooled"
    assert not torch.equal(out[0], out[1]) and not torch.equal(pooled[0], pooled[1])


def _tail_block(C, dev, seed):
    s = 1.0 / math.sqrt(C)
    return dict(w3=rnd(C, C, dev=dev, seed=seed + 1, scale=s), b3=rnd(C, dev=dev, seed=seed + 2, scale=0.1),
                w4=rnd(2 * C, C, dev=dev, seed=seed + 3, scale=s), b4=rnd(2 * C, dev=dev, seed=seed + 4, scale=0.1),
                w5=rnd(C, C, dev=dev, seed=seed + 5, scale=s), b5=rnd(C, dev=dev, seed=seed + 6, scale=0.1),
                beta=rnd(C, dev=dev, seed=seed + 8) * 0.4, gamma=rnd(C, dev=dev, seed=seed + 9) * 0.3,
                ln_g=rnd(C, dev=dev, seed=seed + 10) * 0.1 + 1, ln_b=rnd(C, dev=dev, seed=seed + 11) * 0.1)


# C = 64 [3,16,16]: two 128-row tiles per image; [2,192,192]: 288 tiles per image, 576 > 512 persistent workgroups, so a workgroup walks
# from image 0 into image 1.  C = 128 [3,8,8]: 64 rows per image, image boundaries inside a 128-row tile; [2,128,144]: 288 tiles > 256
@pytest.mark.parametrize("C,B,H,W", [(64, 3, 16, 16), (64, 2, 192, 192), (128, 3, 8, 8), (128, 2, 128, 144)])
def test_naf_tail_batch_equals_single_calls(dev, bf16_mode, C, B, H, W):
    from isr2_amd import ops
    from isr2_amd.prep import pack_naf_tail
    k = _tail_block(C, dev, 300 + C + H)
    pk = pack_naf_tail(k["w3"], k["b3"], k["w4"], k["b4"], k["w5"], k["b5"])
    g = rnd(B, H, W, C, dev=dev, seed=301 + C + H, scale=1.2)
    x = rnd(B, H, W, C, dev=dev, seed=302 + C + H, scale=1.5) + 0.2
    sca = (rnd(B, C, dev=dev, seed=303 + C + H) * 0.3 + 1.0).contiguous()
    assert not torch.equal(sca[0], sca[1])
    out = ops.naf_tail(g, x, pk, sca, k["beta"], k["ln_g"], k["ln_b"], k["gamma"])
    assert tuple(out.shape) == (B, H, W, C)
    for b in range(B):
        o1 = ops.naf_tail(g[b:b + 1], x[b:b + 1], pk, sca[b].contiguous(), k["beta"], k["ln_g"], k["ln_b"], k["gamma"])
        assert torch.equal(out[b:b + 1], o1), f"image {b}"
    # the scale really is per image: image 1 under image 0's vector is something else
    o_wrong = ops.naf_tail(g[1:2], x[1:2], pk, sca[0].contiguous(), k["beta"], k["ln_g"], k["ln_b"], k["gamma"])
    assert not torch.equal(out[1:2], o_wrong) and not torch.equal(out[0], out[1])


# one row per image; four rows; 384 rows = three m-tiles per image; N = K = 1024
@pytest.mark.parametrize("B,H,W,K", [(3, 1, 1, 256), (3, 2, 2, 256), (2, 16, 24, 256), (2, 4, 4, 1024)])
def test_linear_kmul_per_image_equals_single_calls(dev, mode, B, H, W, K):
    """conv3 of the deep levels: bf16x3 goes through the implicit GEMM, bf16 through the bf16-rows GEMM (rows_gemm=True)."""
    from isr2_amd import ops
    N = K
    rows = mode == "bf16"
    x = rnd(B, H, W, K, dev=dev, seed=400 + K + H, scale=1.1)
    res = rnd(B, H, W, N, dev=dev, seed=401 + K + H)
    w, bias = rnd(N, K, dev=dev, seed=402 + K + H, scale=1.0 / math.sqrt(K)), rnd(N, dev=dev, seed=403 + K + H, scale=0.1)
    beta = rnd(N, dev=dev, seed=404 + K + H) * 0.4
    kmul = (rnd(B, K, dev=dev, seed=405 + K + H) * 0.3 + 1.0).contiguous()
    out = ops.linear(x, w, bias, res=res, mul=beta, kmul=kmul, rows_gemm=rows)
    assert tuple(out.shape) == (B, H, W, N)
    for b in range(B):
        o1 = ops.linear(x[b:b + 1], w, bias, res=res[b:b + 1], mul=beta, kmul=kmul[b].contiguous(), rows_gemm=rows)
        assert torch.equal(out[b:b + 1], o1), f"image {b}"
    o_wrong = ops.linear(x[1:2], w, bias, res=res[1:2], mul=beta, kmul=kmul[0].contiguous(), rows_gemm=rows)
    assert not torch.equal(out[1:2], o_wrong) and not torch.equal(out[0], out[1])


def test_refusals_come_before_any_launch(dev, synth_sd):
    from isr2_amd import lib, ops
    from isr2_amd.experts import NafnetHIP
    from isr2_amd.prep import pack_naf_tail
    prev = ops.gemm_mode()
    k = _tail_block(64, dev, 510)
    pk = pack_naf_tail(k["w3"], k["b3"], k["w4"], k["b4"], k["w5"], k["b5"])
    naf = NafnetHIP(synth_sd, dev)
    try:
        with ops.profile() as prof:                                           # (the wrappers raise before they allocate or launch)
            for m, rows in (("bf16x3", False), ("bf16", True)):
                ops.set_gemm_mode(m)
                x = rnd(5, 256, dev=dev, seed=500)                            # 5 rows, kmul of 2 images
                with pytest.raises(lib.FFError):
                    ops.linear(x, rnd(256, 256, dev=dev, seed=501), None, kmul=torch.ones(2, 256, device=dev), rows_gemm=rows)
            ops.set_gemm_mode("bf16")
            g, x = rnd(2, 8, 8, 64, dev=dev, seed=511), rnd(2, 8, 8, 64, dev=dev, seed=512)
            with pytest.raises(lib.FFError):                                  # sca of three images on a tensor of two
                ops.naf_tail(g, x, pk, torch.ones(3, 64, device=dev), k["beta"], k["ln_g"], k["ln_b"], k["gamma"])
            with pytest.raises(lib.FFError):                                  # taps are recorded for B == 1 only
                naf.forward(torch.rand(2, 3, 4, 4, device=dev), taps={})
        assert prof.records() == []
    finally:
        ops.set_gemm_mode(prev)
