"""The fusion stack's ops on a batch: every batched call against B single calls on the sliced images, torch.equal throughout (the
contract is bit identity with the single-image path).  The images of a batch differ, and two outputs of a batch are checked to differ.
Shapes are the smallest at which a route or an indexing mistake can show: 8x8 the minimum of the DCT, 17x19 odd sizes (reflect tails,
the odd-W c2r branch, image bases that are not 16-byte aligned), 20x40 non-square, 64x64 a split column pass of the FFT."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = ["bf16x3", "bf16"]
SIZES = [(8, 8), (17, 19), (20, 40), (64, 64)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(params=MODES)
def mode(request):
    from isr2_amd import ops
    prev = ops.gemm_mode()
    ops.set_gemm_mode(request.param)
    yield request.param
    ops.set_gemm_mode(prev)


@pytest.fixture(scope="module")
def fus(dev):
    from isr2_amd.fusion import FusionHIP
    from isr2_amd.weights import synth_state_dict
    return FusionHIP(synth_state_dict(1234, parts=("fusion",)), dev)


def _rand(seed, *shape, dev):
    return torch.from_numpy(np.random.default_rng(seed).random(shape, dtype=np.float32)).to(dev)


def _randn(seed, *shape, dev, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)).to(dev)


def _differ(t):
    assert not torch.equal(t[0], t[1]), "the images of the batch must differ"


# ---- the three operator families that were single-image at the C ABI --------------------------------------------------------------
@pytest.mark.parametrize("h,w", SIZES)
def test_dct8_bands_batch_equals_single_calls(dev, fus, h, w):
    from isr2_amd import ops
    fb, B = fus.bands, 3
    lr = _rand(10 + h, B, 3, h, w, dev=dev)
    got = torch.full((B, h, w, 27), -7.0, device=dev)
    ops.dct8_bands(lr, fb.dct, fb.masks, fb.dct_scale, got, 0)
    for b in range(B):
        one = torch.full((1, h, w, 27), -7.0, device=dev)
        ops.dct8_bands(lr[b], fb.dct, fb.masks, fb.dct_scale, one, 0)
        assert torch.equal(got[b], one[0]), f"image {b}"
    assert bool((got[..., 9:] == -7.0).all()) and not bool((got[..., :9] == -7.0).any())
    _differ(got)
    # a channel slice of a wider buffer at another offset: the neighbours keep the sentinel
    wide = torch.full((B, h, w, 40), -7.0, device=dev)
    ops.dct8_bands(lr, fb.dct, fb.masks, fb.dct_scale, wide[..., 4:31], 2)
    assert torch.equal(wide[..., 6:15], got[..., :9])
    assert bool((wide[..., :6] == -7.0).all()) and bool((wide[..., 15:] == -7.0).all())


@pytest.mark.parametrize("h,w", SIZES)
def test_fft_bands_batch_equals_single_calls(dev, fus, h, w):
    from isr2_amd import ops
    fb, B = fus.bands, 3
    lr = _rand(20 + h, B, 3, h, w, dev=dev)
    args = (fb._twiddle(w), fb._twiddle(h), fb.mask_logits, fb.temp, fb.fft_scale)
    got = torch.full((B, h, w, 27), -7.0, device=dev)
    ops.fft_bands(lr, *args, got, 21, 24)
    for b in range(B):
        one = torch.full((1, h, w, 27), -7.0, device=dev)
        ops.fft_bands(lr[b], *args, one, 21, 24)
        assert torch.equal(got[b], one[0]), f"image {b}"
    assert bool((got[..., :21] == -7.0).all()) and not bool((got[..., 21:] == -7.0).any())
    _differ(got)
    wide = torch.full((B, h, w, 40), -7.0, device=dev)
    ops.fft_bands(lr, *args, wide[..., 4:31], 5, 1)              # low band after the high band, both inside the slice
    assert torch.equal(wide[..., 9:12], got[..., 21:24]) and torch.equal(wide[..., 5:8], got[..., 24:27])
    assert bool((wide[..., :5] == -7.0).all()) and bool((wide[..., 8] == -7.0).all()) and bool((wide[..., 12:] == -7.0).all())


@pytest.mark.parametrize("h,w", SIZES)
def test_fuse_blend_batch_equals_single_calls(dev, h, w):
    from isr2_amd import ops
    B = 3
    E, hier = _rand(30 + h, B, 4 * h, 4 * w, 9, dev=dev), _rand(31 + h, B, 4 * h, 4 * w, 3, dev=dev)
    guide, gates, dif = _rand(32 + h, B, h, w, 3, dev=dev), _rand(33 + h, B, h, w, 3, dev=dev), _rand(34 + h, B, h, w, 1, dev=dev)
    got = ops.fuse_blend(E, hier, guide, gates, dif)
    assert tuple(got.shape) == (B, 4 * h, 4 * w, 3)
    for b in range(B):
        s = slice(b, b + 1)
        assert torch.equal(got[s], ops.fuse_blend(E[s], hier[s], guide[s], gates[s], dif[s])), f"image {b}"
    _differ(got)


@pytest.mark.parametrize("h,w", SIZES)
def test_freq_bands_batch_equals_single_calls(dev, fus, h, w):
    """FreqBands as a whole: also the DWT passes over 3 B planes and ops.resize from planar [B,3,.,.] into channel slices."""
    B = 3
    lr = _rand(40 + h, B, 3, h, w, dev=dev)
    got = fus.bands(lr)
    assert tuple(got.shape) == (B, h, w, 27)
    for b in range(B):
        assert torch.equal(got[b:b + 1], fus.bands(lr[b:b + 1].clone())), f"image {b} (an aligned copy)"
        assert torch.equal(got[b:b + 1], fus.bands(lr[b:b + 1])), f"image {b} (in place: the base is at b * 3 h w floats)"
    _differ(got)


# ---- what the stack already called with B or a row count: the hints and the routes ------------------------------------------------
def test_linear_rows_per_image_takes_one_images_tile(dev, mode):
    """N = K = 192 on aligned rows, 4096 rows per image, B = 5: one image's M (4096) is below 256 * 64, the batch's (20480) above it, so
    without the hint the batch takes tile configuration 4 where one image takes 7."""
    from isr2_amd import ops
    L = ops._L()
    assert L.ff_conv2d_bf16s_tile(4096, 192, 192, 1) == 7 and L.ff_conv2d_bf16s_tile(5 * 4096, 192, 192, 1) == 4
    B, R = 5, 4096
    x = _randn(50, B, 64, 64, 192, dev=dev)
    w, bias, res = _randn(51, 192, 192, dev=dev, scale=0.1), _randn(52, 192, dev=dev), _randn(53, B, 64, 64, 192, dev=dev)
    got = ops.linear(x, w, bias, act="gelu", res=res, rows_per_image=R)
    for b in range(B):
        s = slice(b, b + 1)
        assert torch.equal(got[s], ops.linear(x[s], w, bias, act="gelu", res=res[s])), f"image {b}"
    _differ(got)
    assert torch.equal(ops.linear(x[:1], w, bias, rows_per_image=R), ops.linear(x[:1], w, bias))       # one image: nothing changes
    with pytest.raises(ops._lib.FFError):
        ops.linear(x, w, bias, rows_per_image=R - 1)


@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("cin,cout", [(76, 64), (9, 64), (96, 32), (6, 8)])
def test_conv2d_per_image_equals_single_calls(dev, mode, cin, cout, H):
    """The 3x3 shapes of the stack on both sides of the route thresholds (the halo route from 1024 pixels, the small-channel VALU route
    from 4096): 76 -> 64 (concat buffer), 9 -> 64, 96 -> 32 (edge features), 6 -> 8 (edge gate)."""
    from isr2_amd import ops
    from isr2_amd.prep import pack_conv
    B = 3
    x = _randn(60 + cin, B, H, H, cin, dev=dev)                   # the pitch the stack has: 76, 9, 96, 6
    w, bias = pack_conv(_randn(61 + cin, cout, cin, 3, 3, dev=dev, scale=0.1).cpu()).to(dev), _randn(62, cout, dev=dev)
    got = ops.conv2d(x, w, bias, ksize=(3, 3), pad=(1, 1), act="gelu", per_image=True)
    for b in range(B):
        s = slice(b, b + 1)
        assert torch.equal(got[s], ops.conv2d(x[s], w, bias, ksize=(3, 3), pad=(1, 1), act="gelu")), f"image {b}"
    _differ(got)


@pytest.mark.parametrize("h,w", [(16, 16), (20, 40)])
def test_lka_depthwise_chain_batch_equals_single_calls(dev, fus, h, w):
    """5x5, 1x21, 21x1 at C = 576: a 21-wide tap must not reach into the neighbouring image."""
    from isr2_amd import ops
    xb, B = fus.xband, 2
    x = _randn(70 + h, B, h, w, 576, dev=dev)

    def chain(t):
        a = ops.dwconv2d(t, xb.dw5, None, ksize=(5, 5), pad=(2, 2))
        a = ops.dwconv2d(a, xb.dwh, None, ksize=(1, 21), pad=(0, 10))
        return ops.dwconv2d(a, xb.dwv, None, ksize=(21, 1), pad=(10, 0))

    got = chain(x)
    for b in range(B):
        assert torch.equal(got[b:b + 1], chain(x[b:b + 1])), f"image {b}"
    _differ(got)


@pytest.mark.parametrize("h,w", [(8, 8), (17, 19)])
def test_mix2_per_image_channel_scale_equals_single_calls(dev, h, w):
    """ff_mix2_images: the cached-mode collaborative gains [B,3] on channel slices of the 9-channel expert tensor, in place."""
    from isr2_amd import ops
    B = 3
    e9 = _rand(80 + h, B, h, w, 9, dev=dev) * 1.5
    ca = _rand(81 + h, B, 3, dev=dev) + 0.5
    want = e9.clone()
    for b in range(B):
        ops.mix2(want[b:b + 1, ..., 3:6], ca=ca[b], clamp01=True, out=want[b:b + 1, ..., 3:6])
    got = e9.clone()
    ops.mix2(got[..., 3:6], ca=ca, clamp01=True, out=got[..., 3:6])
    assert torch.equal(got, want)
    assert torch.equal(got[..., :3], e9[..., :3]) and torch.equal(got[..., 6:], e9[..., 6:]) and not torch.equal(got[..., 3:6], e9[..., 3:6])
    _differ(got[..., 3:6])
    with pytest.raises(ops._lib.FFError):
        ops.mix2(got[..., 3:6], ca=_rand(82, B, 4, dev=dev), out=got[..., 3:6])  # a scale matrix of another channel count
