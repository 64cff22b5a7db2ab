"""The per-image forms a batched DAT forward rests on, each against B single-image calls, bit for bit (torch.equal: the contract is bit
identity with the single-image path, so there is no tolerance): ff_chan_attn_finish_images behind one ff_chan_qkv call, the per-image
weight form of the implicit GEMM, ff_pool_partials_images + ff_pool_vec_mlp_images, ff_token_linear_gated_images -- and what DAT already
called with a B argument (its window attention form, the depth-wise strip kernels, the SGFN tail), pinned so that no row of one image
enters another's window or halo."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = ["bf16x3", "bf16"]
C = 180


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
    """Replace ops._L() by a proxy that counts what reaches the named C entry points (as in tests/test_batched_ops_gpu.py)."""
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


def _rows(shape, dev, seed, scale=1.0, shift=0.0):
    """fp32 rows in the buffers DAT uses: the padded pitch of ops.empty_rows (180 -> 192, 720 -> 736)."""
    from isr2_amd import ops
    t = ops.empty_rows(tuple(shape), dev)
    t.copy_(rnd(*shape, dev=dev, seed=seed, scale=scale) + shift)
    return t


# ---- channel attention: one ff_chan_qkv call for the batch, per-image reduction of its partials ------------------------------------
# blocks per image: 1; 3; 9 (more than the 8 slices of chan_reduce); 25 (the smallest count that enters its four-accumulator loop)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("H,W", [(16, 16), (16, 48), (48, 48), (80, 80)])
def test_chan_qkv_attn_batch_equals_single_calls(dev, monkeypatch, mode, H, W):
    from isr2_amd.prep import pack_chan_qkv
    B, heads = 3, 6
    g, b = (rnd(C, dev=dev, seed=701) * 0.1 + 1).contiguous(), (rnd(C, dev=dev, seed=702) * 0.1).contiguous()
    pk = pack_chan_qkv(rnd(3 * C, C, dev=dev, seed=703, scale=1.0 / math.sqrt(C)), rnd(3 * C, dev=dev, seed=704, scale=0.1))
    temp = (rnd(heads, dev=dev, seed=705) * 0.2 + 1.0).contiguous()
    with _Mode(mode) as ops:
        x = _rows((B, H, W, C), dev, 700 + H + W, scale=1.4, shift=0.2)
        calls = _spy(monkeypatch, ("ff_chan_qkv", "ff_chan_attn_finish", "ff_chan_attn_finish_images"))
        v, wbd = ops.chan_qkv_attn(x, pk, g, b, temp)
        assert calls == ["ff_chan_qkv", "ff_chan_attn_finish_images"], calls
        assert tuple(v.shape) == (B, H, W, C) and tuple(wbd.shape) == (B, C, C)
        for i in range(B):
            del calls[:]
            v1, w1 = ops.chan_qkv_attn(x[i:i + 1], pk, g, b, temp)
            assert calls == ["ff_chan_qkv", "ff_chan_attn_finish"], calls
            assert tuple(w1.shape) == (C, C)
            assert torch.equal(v[i:i + 1], v1), f"image {i}: v"
            assert torch.equal(wbd[i], w1), f"image {i}: attention matrix"
        assert not torch.equal(wbd[0], wbd[1]) and not torch.equal(v[0], v[1])


def test_chan_qkv_attn_batch_refuses_before_any_launch(dev, monkeypatch):
    from isr2_amd.lib import FFError
    from isr2_amd.prep import pack_chan_qkv
    pk = pack_chan_qkv(rnd(3 * C, C, dev=dev, seed=703, scale=0.1), rnd(3 * C, dev=dev, seed=704, scale=0.1))
    v = rnd(C, dev=dev, seed=1)
    with _Mode("bf16x3") as ops:
        calls = _spy(monkeypatch, ("ff_chan_qkv", "ff_chan_attn_finish", "ff_chan_attn_finish_images"))
        with pytest.raises(FFError):                                  # 15 x 17 = 255 tokens per image
            ops.chan_qkv_attn(_rows((2, 15, 17, C), dev, 2), pk, v, v, v[:6].contiguous())
        assert calls == []


# ---- att = v . wbd^T with one matrix per image -----------------------------------------------------------------------------------------
# 3 x 256 rows: the 128 x 64 tile, two m-tiles per image.  2 x 16 384 rows: where ONE image's row count selects the 256 x 192 tile.
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,R", [(3, 256), (2, 16384)])
def test_linear_per_image_weights_equals_single_calls(dev, monkeypatch, mode, B, R):
    from isr2_amd.lib import load
    with _Mode(mode) as ops:
        assert load().ff_conv2d_bf16s_tile(R, C, C, 1) == (4 if R >= 16384 else 7)
        v = _rows((B, R, C), dev, 710 + B)
        wbd = torch.softmax(rnd(B, C, C, dev=dev, seed=711), dim=-1).contiguous()
        calls = _spy(monkeypatch, ("ff_conv2d_bf16s", "ff_conv2d_bf16s_wimages", "ff_split_bf16"))
        got = ops.linear(v, wbd, dynamic_w=True)
        assert calls == ["ff_split_bf16", "ff_conv2d_bf16s_wimages"], calls      # one split of [B * 180, 180], one GEMM
        assert tuple(got.shape) == (B, R, C)
        for i in range(B):
            for w in (wbd[i], wbd[i:i + 1]):                          # [N,K] and [1,N,K]: the single-weight entry point, as before
                del calls[:]
                want = ops.linear(v[i:i + 1], w.contiguous(), dynamic_w=True)
                assert calls == ["ff_split_bf16", "ff_conv2d_bf16s"], calls
                assert torch.equal(got[i:i + 1], want), f"image {i}"
        assert not torch.equal(got[1:2], ops.linear(v[1:2], wbd[0].contiguous(), dynamic_w=True))    # image 1 did not take image 0's matrix


def test_linear_per_image_weights_refuses_before_any_launch(dev, monkeypatch):
    from isr2_amd.lib import FFError
    with _Mode("bf16x3") as ops:
        calls = _spy(monkeypatch, ("ff_conv2d_bf16s", "ff_conv2d_bf16s_wimages", "ff_split_bf16"))
        w2, w3 = rnd(2, C, C, dev=dev, seed=3), rnd(3, C, C, dev=dev, seed=3)
        with pytest.raises(FFError):                                  # 255 rows per image
            ops.linear(_rows((2, 255, C), dev, 4), w2, dynamic_w=True)
        with pytest.raises(FFError):                                  # three matrices for 512 rows
            ops.linear(_rows((2, 256, C), dev, 4), w3, dynamic_w=True)
        with pytest.raises(FFError):                                  # a cached (static) weight has no per-image form
            ops.linear(_rows((2, 256, C), dev, 4), w2)
        with pytest.raises(FFError):
            ops.linear(_rows((2, 256, C), dev, 4), w2, dynamic_w=True, act="gelu")
        assert calls == []


# ---- pool partials of a batch, then the channel-gate MLP ---------------------------------------------------------------------------------
# P = 256: one partial row per image.  P = 6 400 (80 x 80): 25 rows of 256 pixels.
@pytest.mark.parametrize("H,W", [(16, 16), (80, 80)])
def test_pool_partials_and_vec_mlp_batch_equal_single_calls(dev, monkeypatch, H, W):
    from isr2_amd import ops
    from isr2_amd.lib import load
    B, Ch = 3, 11
    x = _rows((B, H, W, C), dev, 720 + H)
    w1, b1 = rnd(Ch, C, dev=dev, seed=721, scale=1.0 / math.sqrt(C)), rnd(Ch, dev=dev, seed=722, scale=0.1)
    w2, b2 = rnd(C, Ch, dev=dev, seed=723, scale=0.4), rnd(C, dev=dev, seed=724, scale=0.1)
    calls = _spy(monkeypatch, ("ff_pool_partials", "ff_pool_partials_images", "ff_pool_mean", "ff_pool_vec_mlp", "ff_pool_vec_mlp_images"))
    pp = ops.pool_partials(x)
    cm = ops.vec_mlp(pp, w1, b1, "gelu", w2, b2, "sigmoid")
    assert calls == ["ff_pool_partials_images", "ff_pool_vec_mlp_images"], calls
    one = load().ff_pool_partial_rows(H * W)
    assert isinstance(pp, ops.PoolPartials) and pp.images == B and pp.rows_per_image == one == (H * W) // 256
    assert tuple(pp.part.shape) == (B * one, C) and tuple(cm.shape) == (B, C)
    for i in range(B):
        del calls[:]
        pp1 = ops.pool_partials(x[i:i + 1])
        cm1 = ops.vec_mlp(pp1, w1, b1, "gelu", w2, b2, "sigmoid")
        assert calls == ["ff_pool_partials", "ff_pool_vec_mlp"], calls
        assert torch.equal(pp.part[i * one:(i + 1) * one], pp1.part), f"image {i}: partial rows"
        assert torch.equal(cm[i:i + 1], cm1), f"image {i}: gate"
        assert torch.equal(pp.mean()[i:i + 1], pp1.mean()), f"image {i}: finished pool"
    assert not torch.equal(cm[0], cm[1]) and not torch.equal(pp.part[:one], pp.part[one:2 * one])


# ---- the gated projection with one channel gate per image ------------------------------------------------------------------------------
def _gated_weights(dev):
    from isr2_amd.prep import pack_token_linear_gated
    Hd = 11
    return pack_token_linear_gated(rnd(C, C, dev=dev, seed=807, scale=1.0 / math.sqrt(C)), rnd(C, dev=dev, seed=808, scale=0.1),
                                   rnd(Hd, C, dev=dev, seed=804, scale=1.0 / math.sqrt(C)), rnd(Hd, dev=dev, seed=805, scale=0.1),
                                   rnd(1, Hd, dev=dev, seed=806, scale=0.5))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,R", [(3, 256), (2, 768)])                 # one workgroup per image; three per image
def test_token_linear_gated_per_image_gate_equals_single_calls(dev, monkeypatch, mode, B, R):
    pk = _gated_weights(dev)
    with _Mode(mode) as ops:
        sp, ch, res = _rows((B, R, C), dev, 800), _rows((B, R, C), dev, 801), _rows((B, R, C), dev, 802)
        cm = torch.sigmoid(rnd(B, C, dev=dev, seed=803)).contiguous()
        assert not torch.equal(cm[0], cm[1])
        calls = _spy(monkeypatch, ("ff_token_linear_gated", "ff_token_linear_gated_images"))
        got = ops.token_linear_gated(sp, ch, pk, cm, 0.13, res=res)
        assert calls == ["ff_token_linear_gated_images"], calls
        assert tuple(got.shape) == (B, R, C)
        for i in range(B):
            for c in (cm[i], cm[i:i + 1]):                            # [K] and [1,K]: the single-gate entry point, as before
                del calls[:]
                want = ops.token_linear_gated(sp[i:i + 1], ch[i:i + 1], pk, c.contiguous(), 0.13, res=res[i:i + 1])
                assert calls == ["ff_token_linear_gated"], calls
                assert torch.equal(got[i:i + 1], want), f"image {i}"
        assert not torch.equal(got[1:2], ops.token_linear_gated(sp[1:2], ch[1:2], pk, cm[0].contiguous(), 0.13, res=res[1:2]))


def test_token_linear_gated_per_image_gate_refuses_before_any_launch(dev, monkeypatch):
    from isr2_amd.lib import FFError
    pk = _gated_weights(dev)
    with _Mode("bf16x3") as ops:
        calls = _spy(monkeypatch, ("ff_token_linear_gated", "ff_token_linear_gated_images"))
        sp, ch = _rows((2, 255, C), dev, 810), _rows((2, 255, C), dev, 811)
        with pytest.raises(FFError):                                  # 255 rows per image: a workgroup would straddle two images
            ops.token_linear_gated(sp, ch, pk, rnd(2, C, dev=dev, seed=812), 0.13)
        sp, ch = _rows((2, 256, C), dev, 810), _rows((2, 256, C), dev, 811)
        for bad in (rnd(3, C, dev=dev, seed=812), rnd(2, C + 4, dev=dev, seed=812), rnd(2, 2, C, dev=dev, seed=812), rnd(C, 2, dev=dev, seed=812),
                    rnd(2, 2 * C, dev=dev, seed=812)[:, :C]):        # three gates for two images; wrong widths / ranks; rows that are not contiguous
            with pytest.raises(FFError):
                ops.token_linear_gated(sp, ch, pk, bad, 0.13)
        assert calls == []


# ---- what DAT already called with a B argument ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shifted", [False, True])
def test_win_attn_fused_dat_form_batch_equals_single_calls(dev, mode, shifted):
    """DAT's form of the fused window attention: half the heads per launch, 8 x 32 and 32 x 8 windows on a 16 x 48 image zero-padded
    to 32 x 64 (Hp > H, Wp > W), both halves of v written as a side output."""
    from isr2_amd.prep import pack_win_attn, pack_win_rel
    B, H, W, heads, d = 2, 16, 48, 6, 30
    hh = heads // 2
    Hp, Wp = 32, 64
    pk = pack_win_attn(rnd(3 * C, C, dev=dev, seed=820, scale=1.0 / math.sqrt(C)), rnd(3 * C, dev=dev, seed=821, scale=0.1), heads, d, d ** -0.5)
    g, b = (rnd(C, dev=dev, seed=822) * 0.1 + 1).contiguous(), (rnd(C, dev=dev, seed=823) * 0.1).contiguous()
    with _Mode(mode) as ops:
        x = _rows((B, H, W, C), dev, 824, shift=0.1)

        def run(xs):
            att, v = ops.empty_like_rows(xs), ops.empty_like_rows(xs)
            att.fill_(-7.0)
            v.fill_(-7.0)
            for br, (wh, ww) in enumerate(((8, 32), (32, 8))):
                r6 = torch.zeros(heads, (2 * wh - 1) * (2 * ww - 1), device=dev)
                r6[hh * br:hh * br + hh] = rnd(hh, (2 * wh - 1) * (2 * ww - 1), dev=dev, seed=825 + br, scale=0.5)
                ops.win_attn_fused(xs, att, pk, pack_win_rel(r6, wh, ww), gamma=g, beta=b, H=H, W=W, Hp=Hp, Wp=Wp, win=(wh, ww),
                                   shift=(wh // 2, ww // 2) if shifted else (0, 0), use_mask=shifted, head0=hh * br, nheads=hh, zero_pad=True,
                                   v_out=v, v_off=0)
            return att, v

        att, v = run(x)
        assert not bool((att == -7.0).any()) and not bool((v == -7.0).any())       # every token of every image was written
        for i in range(B):
            a1, v1 = run(x[i:i + 1])
            assert torch.equal(att[i:i + 1], a1), f"image {i}: attention output"
            assert torch.equal(v[i:i + 1], v1), f"image {i}: v side output"
        assert not torch.equal(att[0], att[1]) and not torch.equal(v[0], v[1])


@pytest.mark.parametrize("H,W", [(16, 48), (32, 32)])
def test_dwconv_strip_kernels_batch_equal_single_calls(dev, H, W):
    """ff_dwconv2d's 3x3 strip kernel (DAT's conv branch: + BN + GELU) and ff_dwconv3x3_ln (the SpatialGate of the bf16x3 route): the first
    and last rows of an image take zeros, not the neighbouring image's rows."""
    from isr2_amd import ops
    from isr2_amd.prep import pack_dw
    B, c2 = 2, 360
    x = _rows((B, H, W, C), dev, 830)
    wd, bd = pack_dw(rnd(C, 1, 3, 3, dev=dev, seed=831, scale=0.3)), rnd(C, dev=dev, seed=832, scale=0.1)
    sc, sh = (rnd(C, dev=dev, seed=833) * 0.1 + 1).contiguous(), (rnd(C, dev=dev, seed=834) * 0.1).contiguous()
    got = ops.dwconv2d(x, wd, bd, post_scale=sc, post_shift=sh, act="gelu")
    for i in range(B):
        assert torch.equal(got[i:i + 1], ops.dwconv2d(x[i:i + 1], wd, bd, post_scale=sc, post_shift=sh, act="gelu")), f"image {i}: dwconv2d"
    assert not torch.equal(got[0], got[1])
    y = _rows((B, H, W, 2 * c2), dev, 835)                             # fc1's output: x1 | x2 at a pitch of 736
    stats = torch.stack((rnd(B * H * W, dev=dev, seed=836, scale=0.2), rnd(B * H * W, dev=dev, seed=837).abs() + 0.5), dim=1).contiguous()
    w2, b2 = pack_dw(rnd(c2, 1, 3, 3, dev=dev, seed=838, scale=0.3)), rnd(c2, dev=dev, seed=839, scale=0.1)
    g2, bb2 = (rnd(c2, dev=dev, seed=840) * 0.1 + 1).contiguous(), (rnd(c2, dev=dev, seed=841) * 0.1).contiguous()
    z = ops.dwconv3x3_ln(y[..., c2:], w2, b2, stats, g2, bb2, mul_in=y[..., :c2])
    for i in range(B):
        z1 = ops.dwconv3x3_ln(y[i:i + 1, ..., c2:], w2, b2, stats[i * H * W:(i + 1) * H * W], g2, bb2, mul_in=y[i:i + 1, ..., :c2])
        assert torch.equal(z[i:i + 1], z1), f"image {i}: dwconv3x3_ln"
    assert not torch.equal(z[0], z[1])


@pytest.mark.parametrize("H,W", [(16, 48), (32, 32)])
def test_sgfn_tail_batch_equals_single_calls(dev, H, W):
    """ff_sgfn_tail (plain bf16): the halo rows above an image's first row and below its last are zeros of the normalised tensor."""
    from isr2_amd.prep import pack_dw
    B, c2 = 2, 360
    with _Mode("bf16") as ops:
        y = _rows((B, H, W, 2 * c2), dev, 850)
        res = _rows((B, H, W, C), dev, 851)
        stats = torch.stack((rnd(B * H * W, dev=dev, seed=852, scale=0.2), rnd(B * H * W, dev=dev, seed=853).abs() + 0.5), dim=1).contiguous()
        wd, bd = pack_dw(rnd(c2, 1, 3, 3, dev=dev, seed=854, scale=0.3)), rnd(c2, dev=dev, seed=855, scale=0.1)
        g2, bb2 = (rnd(c2, dev=dev, seed=856) * 0.1 + 1).contiguous(), (rnd(c2, dev=dev, seed=857) * 0.1).contiguous()
        w2, b2 = rnd(C, c2, dev=dev, seed=858, scale=1.0 / math.sqrt(c2)), rnd(C, dev=dev, seed=859, scale=0.1)
        got = ops.sgfn_tail(y, c2, wd, bd, stats, g2, bb2, w2, b2, res=res)
        for i in range(B):
            want = ops.sgfn_tail(y[i:i + 1], c2, wd, bd, stats[i * H * W:(i + 1) * H * W], g2, bb2, w2, b2, res=res[i:i + 1])
            assert torch.equal(got[i:i + 1], want), f"image {i}"
        assert not torch.equal(got[0], got[1])
