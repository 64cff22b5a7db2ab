"""The three per-image entry points a batched HAT forward rests on, each against B single-image calls, bit for bit
(torch.equal: the contract is bit identity with the single-image path, so there is no tolerance):
ff_token_projmlp_images (one gate vector per image), ff_conv3x3_halo_images (per-image kernel form and pool partial rows) and
ff_pool_vec_mlp_images (pool finish + channel-attention MLP, one workgroup per image)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rnd(*shape, dev, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


class _Mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from isr2_amd import ops
        self.prev = ops.gemm_mode()
        ops.set_gemm_mode(self.mode)
        return ops

    def __exit__(self, *exc):
        from isr2_amd import ops
        ops.set_gemm_mode(self.prev)


def _spy(monkeypatch, names):
    """Replace ops._L() by a proxy that counts what reaches the named C entry points."""
    from isr2_amd import lib as L, ops
    calls = []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(L.load(), name)
            if name not in names:
                return fn

            def counted(*a):
                calls.append(name)
                return fn(*a)
            return counted

    monkeypatch.setattr(ops, "_L", lambda: Spy())
    return calls


# ---- token_projmlp with one gate per image ---------------------------------------------------------------------------------------
def _projmlp_weights(dev):
    from isr2_amd.prep import pack_token_projmlp
    C, Hd = 180, 360
    pk = pack_token_projmlp(rnd(C, C, dev=dev, seed=950, scale=1.0 / math.sqrt(C)), rnd(C, dev=dev, seed=951, scale=0.1),
                            rnd(Hd, C, dev=dev, seed=952, scale=1.0 / math.sqrt(C)), rnd(Hd, dev=dev, seed=953, scale=0.1),
                            rnd(C, Hd, dev=dev, seed=954, scale=1.0 / math.sqrt(Hd)), rnd(C, dev=dev, seed=955, scale=0.1))
    return pk, (rnd(C, dev=dev, seed=956) * 0.1 + 1).contiguous(), (rnd(C, dev=dev, seed=957) * 0.1).contiguous()


def _rows(B, R, C, dev, seed, bf16):
    """[B,R,C] rows in the buffers HAT uses: padded fp32 pitch (192) or padded bf16 pitch."""
    from isr2_amd import ops
    t = ops.empty_rows_bf16((B, R, C), dev) if bf16 else ops.empty_rows((B, R, C), dev)
    t.copy_(rnd(B, R, C, dev=dev, seed=seed))
    return t


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("B,R", [(3, 256), (2, 768)])                 # one workgroup per image; three per image
def test_token_projmlp_per_image_gate_equals_single_calls(dev, monkeypatch, mode, B, R):
    C = 180
    pk, g, b = _projmlp_weights(dev)
    with _Mode(mode) as ops:
        b16 = mode == "bf16"                                          # plain bf16: att / c2 are the bf16 rows HatHIP.hab stores
        att, c2 = _rows(B, R, C, dev, 960, b16), _rows(B, R, C, dev, 961, b16)
        x = _rows(B, R, C, dev, 962, False)
        scale = (torch.sigmoid(rnd(B, C, dev=dev, seed=963)) * 0.01).contiguous()      # distinct per image
        assert not torch.equal(scale[0], scale[1])
        calls = _spy(monkeypatch, ("ff_token_projmlp", "ff_token_projmlp_images"))
        got = ops.token_projmlp(att, x, pk, g, b, c2=c2, c2_scale=scale)
        assert calls == ["ff_token_projmlp_images"], calls
        assert tuple(got.shape) == (B, R, C)
        for i in range(B):
            for sc in (scale[i], scale[i:i + 1]):                     # [K] and [1,K]: the single-gate entry point, as before
                del calls[:]
                want = ops.token_projmlp(att[i:i + 1], x[i:i + 1], pk, g, b, c2=c2[i:i + 1], c2_scale=sc.contiguous())
                assert calls == ["ff_token_projmlp"], calls
                assert torch.equal(got[i:i + 1], want), f"image {i}"
        assert not torch.equal(got[1], ops.token_projmlp(att[1:2], x[1:2], pk, g, b, c2=c2[1:2], c2_scale=scale[0].contiguous())[0])


def test_token_projmlp_per_image_gate_refuses_before_any_launch(dev, monkeypatch):
    from isr2_amd.lib import FFError, load
    C = 180
    pk, g, b = _projmlp_weights(dev)
    with _Mode("bf16x3") as ops:
        calls = _spy(monkeypatch, ("ff_token_projmlp", "ff_token_projmlp_images"))
        att, c2, x = (_rows(3, 128, C, dev, s, False) for s in (970, 971, 972))
        with pytest.raises(FFError):                                  # an image of 128 rows is half a workgroup
            ops.token_projmlp(att, x, pk, g, b, c2=c2, c2_scale=rnd(3, C, dev=dev, seed=973))
        att, c2, x = (_rows(3, 256, C, dev, s, False) for s in (970, 971, 972))
        with pytest.raises(FFError):                                  # two gates for three images
            ops.token_projmlp(att, x, pk, g, b, c2=c2, c2_scale=rnd(2, C, dev=dev, seed=973))
        assert calls == []
        # the C entry point refuses the same on its own, before its launch
        m = pk["mlp"]
        sc = rnd(3, C, dev=dev, seed=973)
        out = ops.empty_like_rows(x)                                  # pitch 192 like x: torch.empty_like of the view would be compact
        assert out.stride(-2) == x.stride(-2) == 192

        def c_call(nimg, rpi, M, scale_ld=C, c2p=c2.data_ptr(), scp=sc.data_ptr()):
            return load().ff_token_projmlp_images(att.data_ptr(), 192, x.data_ptr(), 192, c2p, 192, scp, scale_ld, nimg, rpi,
                                                  out.data_ptr(), 192, M, C, m["ht"], pk["proj"]["w"].data_ptr(), pk["proj"]["b"].data_ptr(),
                                                  g.data_ptr(), b.data_ptr(), 1e-5, m["w"].data_ptr(), m["b1"].data_ptr(), m["b2"].data_ptr(),
                                                  3, 0, torch.cuda.current_stream().cuda_stream)
        assert c_call(6, 128, 768) != 0 and c_call(2, 256, 768) != 0 and c_call(3, 256, 512) != 0
        assert c_call(3, 256, 768, scale_ld=176) != 0 and c_call(3, 256, 768, scale_ld=182) != 0       # shorter than K; gate rows off 16 bytes
        assert c_call(3, 256, 768, c2p=None) != 0 and c_call(3, 256, 768, scp=None) != 0
        assert c_call(3, 256, 768) == 0
        torch.cuda.synchronize()


# ---- 3x3 halo convolution over B images with per-image pool partials, then the gate ---------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("H,W", [(32, 48), (37, 45)])                 # 1 536 pixels: the smallest grid on the halo route; ragged edge tiles
def test_conv_partials_and_gate_equal_single_image_calls(dev, monkeypatch, mode, H, W):
    from isr2_amd.prep import pack_conv
    B, Cin, Cout = 2, 60, 180
    w = pack_conv(rnd(Cout, Cin, 3, 3, dev=dev, seed=980, scale=1.0 / math.sqrt(9 * Cin)))
    bias = rnd(Cout, dev=dev, seed=981, scale=0.1)
    w1, b1 = rnd(6, Cout, dev=dev, seed=982, scale=1.0 / math.sqrt(Cout)), rnd(6, dev=dev, seed=983, scale=0.1)
    w2, b2 = rnd(Cout, 6, dev=dev, seed=984, scale=0.4), rnd(Cout, dev=dev, seed=985, scale=0.1)
    with _Mode(mode) as ops:
        x = ops.empty_rows((B, H, W, Cin), dev)
        x.copy_(rnd(B, H, W, Cin, dev=dev, seed=986))
        calls = _spy(monkeypatch, ("ff_conv3x3_halo", "ff_conv3x3_halo_images", "ff_pool_vec_mlp", "ff_pool_vec_mlp_images", "ff_conv2d_bf16s"))
        out, pp = ops.conv2d(x, w, bias, ksize=(3, 3), pad=(1, 1), want_pool="partials")
        assert isinstance(pp, ops.PoolPartials) and pp.images == B and pp.part.shape[0] == B * pp.rows_per_image
        gate = ops.vec_mlp(pp, w1, b1, "relu", w2, b2, "sigmoid", post=0.01)
        assert calls == ["ff_conv3x3_halo_images", "ff_pool_vec_mlp_images"], calls
        assert tuple(gate.shape) == (B, Cout) and tuple(pp.mean().shape) == (B, Cout)
        for i in range(B):
            out1, pp1 = ops.conv2d(x[i:i + 1], w, bias, ksize=(3, 3), pad=(1, 1), want_pool="partials")
            assert isinstance(pp1, ops.PoolPartials) and pp1.part.shape[0] == pp.rows_per_image
            assert torch.equal(out[i:i + 1], out1), f"image {i}: output"
            assert torch.equal(pp.part[i * pp.rows_per_image:(i + 1) * pp.rows_per_image], pp1.part), f"image {i}: partial rows"
            assert torch.equal(gate[i:i + 1], ops.vec_mlp(pp1, w1, b1, "relu", w2, b2, "sigmoid", post=0.01)), f"image {i}: gate"
            assert torch.equal(pp.mean()[i:i + 1], pp1.mean()), f"image {i}: finished pool"
        # without pool partials the per-image form stores the same output
        assert torch.equal(ops.conv2d(x, w, bias, ksize=(3, 3), pad=(1, 1), per_image=True), out)


def test_pool_vec_mlp_images_equals_single_launches(dev):
    """The batched finish + MLP against B ff_pool_vec_mlp launches: odd row counts, a padded pitch, the optional pooled output."""
    from isr2_amd.lib import load, check
    B, rows, ld, C, Ch = 3, 37, 192, 180, 6
    part = rnd(B * rows, ld, dev=dev, seed=990)
    w1, b1 = rnd(Ch, C, dev=dev, seed=991, scale=0.1), rnd(Ch, dev=dev, seed=992, scale=0.1)
    w2, b2 = rnd(C, Ch, dev=dev, seed=993, scale=0.4), rnd(C, dev=dev, seed=994, scale=0.1)
    st = torch.cuda.current_stream().cuda_stream
    out, pooled = torch.empty(B, C, device=dev), torch.empty(B, C, device=dev)
    check(load().ff_pool_vec_mlp_images(part.data_ptr(), B, rows, ld, 1.0 / 1536, C, w1.data_ptr(), b1.data_ptr(), Ch, 2, w2.data_ptr(), b2.data_ptr(),
                                        C, 4, 0.01, out.data_ptr(), pooled.data_ptr(), st))
    for i in range(B):
        o1, p1 = torch.empty(1, C, device=dev), torch.empty(1, C, device=dev)
        check(load().ff_pool_vec_mlp(part[i * rows:].data_ptr(), rows, ld, 1.0 / 1536, C, w1.data_ptr(), b1.data_ptr(), Ch, 2, w2.data_ptr(),
                                     b2.data_ptr(), C, 4, 0.01, o1.data_ptr(), p1.data_ptr(), st))
        assert torch.equal(out[i:i + 1], o1) and torch.equal(pooled[i:i + 1], p1), f"image {i}"
    assert not torch.equal(out[0], out[1])


def test_pool_vec_mlp_images_refuses_bad_dims(dev):
    """On device buffers large enough for every case, so that a check that stopped refusing would show as a zero return, not as a fault."""
    from isr2_amd.lib import load
    z = torch.zeros(1 << 16, device=dev)
    p, st = z.data_ptr(), torch.cuda.current_stream().cuda_stream
    for B, rows, ld, Cin, Ch in ((0, 6, 192, 180, 6), (2, 0, 192, 180, 6), (2, 6, 100, 180, 6), (2, 6, 192, 180, 65), (2, 6, 600, 600, 6)):
        assert load().ff_pool_vec_mlp_images(p, B, rows, ld, 1.0, Cin, p, p, Ch, 2, p, p, 180, 4, 1.0, p, None, st) == 1, (B, rows, ld, Cin, Ch)
    torch.cuda.synchronize()
